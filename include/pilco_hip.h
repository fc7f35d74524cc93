/*
 * pilco_hip.h -- C ABI of libpilco_hip.so, the MI355X (gfx950) implementation of
 * the PILCO moment-matching rollout and GP-factorisation hot path.
 *
 * The reference (nrontsis/PILCO) has no FFI layer: its boundary is the Python
 * method surface of pilco.models.MGPR / SMGPR / PILCO.  Each entry point below
 * names the reference method (file:line under /root/reference) whose arithmetic
 * it replaces; pilco_amd/ (Python, ctypes) re-creates that method surface on top
 * of this header, and INTEGRATION.md shows the stub a maintainer of the
 * reference would add.
 *
 * Conventions: every matrix is row-major float64 in caller-owned HOST memory
 * unless a parameter is documented as a device pointer; the library owns all
 * device memory.  A context is bound to one GPU and must be used from one host
 * thread at a time.  Every function returns a pilco_status (0 = OK) and never
 * aborts; pilco_last_error() gives the message for the last failure.
 */
#ifndef PILCO_HIP_H
#define PILCO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* 2: round 6 -- the round-4 persistent-kernel entry points are gone (since round 5) and the launch-structure knobs,
 * the sharding-plan introspection and pilco_rollout_tape are declared in pilco_hip_dev.h (still exported). */
#define PILCO_HIP_ABI_VERSION 2

typedef struct pilco_ctx pilco_ctx;

typedef enum pilco_status {
    PILCO_OK = 0,
    PILCO_E_SHAPE = 1,   /* inconsistent sizes / null pointer */
    PILCO_E_NOT_PD = 2,  /* Cholesky failed: the reference raises InvalidArgumentError (tests/test_cascade.py:22) */
    PILCO_E_HIP = 3,     /* HIP runtime error */
    PILCO_E_RCCL = 4,    /* RCCL error */
    PILCO_E_STATE = 5,   /* call order violated (e.g. predict before set_data) */
    PILCO_E_ALLOC = 6
} pilco_status;

/* ------------------------------------------------------------------ context */
int pilco_abi_version(void);
/* device: HIP device ordinal.  One context per process per GPU. */
int pilco_ctx_create(int device, pilco_ctx** out);
int pilco_ctx_destroy(pilco_ctx* ctx);
const char* pilco_last_error(const pilco_ctx* ctx);
/* index of the output whose Gram matrix was not positive definite (-1 if none) */
int pilco_last_not_pd_output(const pilco_ctx* ctx);
/* checks the f64 MFMA fragment layout assumptions on the device; 0 = OK */
int pilco_selftest(pilco_ctx* ctx);

/* ------------------------------------------------------------------ GP model
 * Slot 0 is the dynamics model (MGPR / SMGPR); slot 1 is the RBF policy
 * (RbfController is an MGPR subclass, pilco/controllers.py:80-129).            */
#define PILCO_SLOT_DYNAMICS 0
#define PILCO_SLOT_POLICY 1

/* MGPR.__init__/set_data (pilco/models/mgpr.py:18-45): X (N,D), Y (N,E).
 * N may change between calls; any cached factorisation is invalidated. */
int pilco_gp_set_data(pilco_ctx* ctx, int slot, const double* X, const double* Y, int N, int D, int E);
/* kernel.lengthscales (E,D), kernel.variance (E), likelihood.variance (E)
 * (properties at pilco/models/mgpr.py:170-186). Invalidates the factorisation. */
int pilco_gp_set_hyp(pilco_ctx* ctx, int slot, const double* lengthscales, const double* variance, const double* noise);
/* SMGPR inducing inputs Z (M,D) of model 0, used for every output
 * (pilco/models/smgpr.py:20-22,47-52).  M = 0 switches back to the exact GP. */
int pilco_gp_set_inducing(pilco_ctx* ctx, int slot, const double* Z, int M);
/* MGPR.K(X1, X2) (pilco/models/mgpr.py:154-157): out (E,N1,N2). X2 may be NULL (= X1). */
int pilco_gp_gram(pilco_ctx* ctx, int slot, const double* X1, int N1, const double* X2, int N2, double* out);
/* MGPR.calculate_factorizations (pilco/models/mgpr.py:81-89) or, when inducing
 * inputs are set, SMGPR.calculate_factorizations (pilco/models/smgpr.py:24-45).
 * Result stays on the device and is cached until data / hyper-parameters change. */
int pilco_gp_factorize(pilco_ctx* ctx, int slot);
/* Negative log marginal likelihood of every output at the current hyper-parameters and its gradient
 * w.r.t. (lengthscales[D], kernel variance, noise variance): what gpflow's GPR.training_loss and its
 * autodiff provide to MGPR.optimize (pilco/models/mgpr.py:47-75), without the prior terms (added on
 * the host).  nlml (E), grad (E, D+2) may be NULL.  Exact GP only.
 * Several ranks: sharded by output like the factorisation under it -- a rank evaluates the outputs it owns; with a
 * communicator attached one ncclAllGather of (D + 3) doubles per output completes the arrays on every rank, without one the
 * other ranks' entries come back NaN and the caller combines them (contexts of one process: pilco_amd._lib.group_nlml). */
int pilco_gp_nlml(pilco_ctx* ctx, int slot, double* nlml, double* grad);
/* The same for the sparse model: negative log marginal likelihood of gpflow's GPRFITC (one model per output, each with its
 * OWN inducing inputs: pilco/models/smgpr.py:16-22) and its gradient w.r.t. (lengthscales[D], kernel variance, noise
 * variance) and w.r.t. the inducing inputs -- what MGPR.optimize's SciPy loop receives for an SMGPR
 * (pilco/models/mgpr.py:47-75; no priors, smgpr.py sets none).  Z_all (E,M,D); nlml (E); grad_hyp (E,D+2) and
 * grad_Z (E,M,D) may be NULL.  Uses the slot's data and hyper-parameters; invalidates its cached factorisation. 
 * Several ranks: sharded by output exactly like pilco_gp_nlml (own outputs evaluated, all-gather with a communicator, NaN for
 * the other ranks' outputs without one). */
int pilco_gp_fitc_nlml(pilco_ctx* ctx, int slot, const double* Z_all, int M, double* nlml, double* grad_hyp, double* grad_Z);
/* number of points the moment-matching runs over: N (exact) or M (sparse) */
int pilco_gp_num_points(const pilco_ctx* ctx, int slot);
/* download iK (E,n,n) and beta (E,n); either may be NULL */
int pilco_gp_get_factors(pilco_ctx* ctx, int slot, double* iK, double* beta);
/* upload caller-supplied factors for predict_given_factorizations(m,s,iK,beta)
 * (pilco/models/mgpr.py:91); iK may be NULL meaning all-zero (RbfController,
 * pilco/controllers.py:116). */
int pilco_gp_set_factors(pilco_ctx* ctx, int slot, const double* iK, const double* beta);
/* MGPR.predict_given_factorizations with the factors held on the device
 * (pilco/models/mgpr.py:91-149): m (1,D), s (D,D) -> M (1,E), S (E,E), V (D,E).
 * pilco_gp_predict = predict_on_noisy_inputs (mgpr.py:77-79) with the
 * factorisation cached instead of recomputed. */
int pilco_gp_predict(pilco_ctx* ctx, int slot, const double* m, const double* s, double* M, double* S, double* V);
/* GPflow GPR.predict_f / GPRFITC.predict_f (full_cov=False) of the model in `slot` at Nt deterministic inputs
 * Xs (Nt, D): latent mean (E, Nt) and latent variance (E, Nt), output-major.  output = -1: all E outputs;
 * 0 <= output < E: that output only (mean, var hold Nt values).  Z_all (sparse slots only, may be NULL):
 * (E, M, D), output e's own inducing inputs; NULL = the slot's Z for every output.
 * Needs the slot's own factorisation (factorises if it is not current; PILCO_E_STATE after pilco_gp_set_factors or on a
 * sharded context) and leaves it unchanged.  Every test point's result is computed in a fixed order that does not depend
 * on the other points of the call: a point gives the same bits alone or in any batch.  Chunked over the test points:
 * bounded memory for any Nt. */
int pilco_gp_predict_points(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int output, const double* Z_all,
                            double* mean, double* var);
/* The same posterior with its derivatives with respect to the test input (extension; docs/predict_jacobians.md):
 *   dmean (E, Nt, D) = d mean_e(x_t) / d x_d,   dvar (E, Nt, D) = d var_e(x_t) / d x_d      (output-major, like mean and var).
 * mean and var may each be NULL; where given they hold the bits pilco_gp_predict_points returns.  Arguments, refusals and
 * chunking as for pilco_gp_predict_points; dmean and dvar must not be NULL.  A test point's derivatives are summed in a
 * fixed order that depends on its own coordinates only: the same bits alone, in any batch and for one output or all. */
int pilco_gp_predict_points_jac(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int output, const double* Z_all,
                                double* mean, double* var, double* dmean, double* dvar);
/* The full posterior covariance between the test points (GPflow predict_f with full_cov=True; docs/predict_cov.md):
 *   cov (E, Nt, Nt), output-major:  cov_e[a][b] = k_e(x_a, x_b) - w_a . w_b,  w_a = L^{-1} k*(x_a)
 *   (FITC: - w0_a . w0_b + sn2 w1_a . w1_b with w0 = Luu^{-1} ku*, w1 = iAt ku*).
 * mean (E, Nt) may be NULL; where given it holds the bits pilco_gp_predict_points returns.  Arguments and refusals as for
 * pilco_gp_predict_points, and PILCO_E_SHAPE when the call's footprint -- (operators + 1) E Ntpad npad doubles of cross-
 * covariances and products plus E Ntpad^2 of covariance, Ntpad = Nt rounded up to 64 -- exceeds the budget (2^30 doubles;
 * environment variable PILCO_PREDICT_COV_BUDGET): the message names the largest Nt that fits.  Not chunked over test points.
 * Bit contracts: cov_e is symmetric to the bit; cov_e[a][b] depends on x_a, x_b and the model only -- not on Nt, not on
 * where the two points stand among the test points, not on whether the output is computed alone or with the others; run to
 * run the bits are identical.  The diagonal agrees with pilco_gp_predict_points' var within rounding, NOT to the bit: that
 * kernel sums the squares in an order of its own. */
int pilco_gp_predict_points_cov(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int output, const double* Z_all,
                                double* mean, double* cov);
/* Joint samples of the latent functions at the test points (GPflow predict_f_samples with full_cov=True):
 *   samples (S, Nt, E):  f[s][a][e] = mean_e[a] + (C_e z[s][.][e])_a,   C_e C_e^T = cov_e + jitter I   (C_e lower triangular).
 * z_in (S, Nt, E) are the caller's standard normals; NULL: drawn on the device, Philox domain 5 -- counter {s, a, j, 5}
 * gives the normals of outputs 2j, 2j + 1 of sample s at test point a, so a draw depends on (seed, s, a, e) only.
 * mean (E, Nt), cov (E, Nt, Nt), chol (E, Nt, Nt: C_e with zeros above the diagonal) and z_out (S, Nt, E: the normals used)
 * are outputs and may each be NULL; for one output (0 <= output < E) read E = 1 in these shapes.  mean and cov hold the
 * bits of pilco_gp_predict_points_cov; a sample's bits do not depend on S.  Everything is enqueued in one pass: one download,
 * one synchronisation.  Refusals of pilco_gp_predict_points_cov (the budget counts three E Ntpad^2 matrices and the
 * normals), PILCO_E_SHAPE for S <= 0 or a jitter that is negative or not finite; PILCO_E_NOT_PD when a pivot of some
 * cov_e + jitter I is not positive (the message names the output, pilco_last_not_pd_output returns it): nothing is written
 * to the caller's arrays then. */
int pilco_gp_sample_points(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int output, const double* Z_all, int S,
                           unsigned long long seed, const double* z_in, double jitter, double* samples, double* mean,
                           double* cov, double* chol, double* z_out);

/* ------------------------------------------------------------------ rollout */
typedef enum pilco_policy_kind {
    PILCO_POLICY_NONE = 0,   /* control_dim == 0 */
    PILCO_POLICY_LINEAR = 1, /* LinearController (pilco/controllers.py:39-63) */
    PILCO_POLICY_RBF = 2,    /* RbfController (pilco/controllers.py:80-129); GP in PILCO_SLOT_POLICY */
    PILCO_POLICY_MLP = 3     /* one-hidden-layer tanh network (extension; docs/particle_mlp.md): particle entry points only; its
                                parameters live in the context (pilco_set_policy_mlp), W and b stay NULL */
} pilco_policy_kind;

typedef struct pilco_policy {
    int kind;
    int state_dim;            /* E of the dynamics model */
    int control_dim;          /* D - E */
    const double* W;          /* linear: (control_dim, state_dim) */
    const double* b;          /* linear: (1, control_dim) */
    const double* max_action; /* (control_dim) scale of squash_sin (controllers.py:13-36); NULL = ones */
    int squash;               /* 1 = apply squash_sin (the reference always does inside propagate) */
} pilco_policy;

typedef enum pilco_reward_kind {
    PILCO_REWARD_EXPONENTIAL = 1, /* ExponentialReward (pilco/rewards.py:7-51) */
    PILCO_REWARD_LINEAR = 2       /* LinearReward (pilco/rewards.py:53-61) */
} pilco_reward_kind;

typedef struct pilco_reward_term {
    int kind;
    double coef;     /* CombinedRewards coefficient (pilco/rewards.py:64-81); 1 for a single reward */
    const double* W; /* exponential: (E,E); linear: (E) */
    const double* t; /* exponential: (1,E) target; NULL = zeros */
} pilco_reward_term;

/* PILCO.predict (pilco/models/pilco.py:118-136) = H x [reward(m,s); propagate
 * (pilco.py:138-153)].  m0 (1,E), S0 (E,E) -> mH (1,E), SH (E,E), reward (sum of
 * the mean rewards of the PRE-propagation states).  traj (optional, may be
 * NULL): (H+1) x (E + E*E) doubles, the state after every step.
 * The factorisation of slot 0 (and slot 1 for an RBF policy) must be current. */
int pilco_rollout(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                  const double* m0, const double* S0, int H, double* mH, double* SH, double* reward, double* traj);
/* B independent rollouts of ONE model in flight together on one GPU: policies [B] (NONE / LINEAR; each lane may have its
 * own parameters), m0 [B][E], S0 [B][E][E] -> mH [B][E], SH [B][E][E], reward [B].  What multi-start policy search and the
 * evaluation of several initial states need (the reference evaluates its restarts one after the other, pilco.py:96-110).
 * Lanes 1..B-1 are internal contexts (own stream, workspace, state, cached graph) that borrow this context's model -- no
 * copy of X / beta / iK; all B graph replays are enqueued before the first wait, so the serial head of one lane's step
 * runs under the pair kernels of the others.  Every lane runs exactly pilco_rollout's launch sequence: its result is
 * BIT-IDENTICAL to its solo run.  Single rank.  More than 4 lanes overlap only if the HIP runtime has as many hardware
 * queues (GPU_MAX_HW_QUEUES, set before the runtime starts). */
int pilco_rollout_batch(pilco_ctx* ctx, int B, const pilco_policy* policies, const pilco_reward_term* rewards, int n_rewards,
                        const double* m0, const double* S0, int H, double* mH, double* SH, double* reward);
/* PILCO.propagate (pilco/models/pilco.py:138-153): one step, no reward. */
int pilco_propagate(pilco_ctx* ctx, const pilco_policy* policy, const double* m_x, const double* s_x, double* M_x, double* S_x);
/* controller.compute_action(m, s, squash) -> M (1,U), S (U,U), V (E,U)
 * (pilco/controllers.py:46-58,108-121) and reward.compute_reward(m,s) ->
 * muR, sR (pilco/rewards.py:19-51,58-61,73-81), evaluated on the device.
 * policy_action bounds state_dim and control_dim separately (each <= 32): state_dim + control_dim may exceed the 32 of a
 * rollout, up to what the link's buffers allow in 160 KB of LDS -- (20, 20) and (32, 8) are supported, (32, 32) is refused
 * with PILCO_E_SHAPE before any launch. */
int pilco_policy_action(pilco_ctx* ctx, const pilco_policy* policy, const double* m, const double* s, double* M, double* S, double* V);
int pilco_reward_eval(pilco_ctx* ctx, const pilco_reward_term* rewards, int n_rewards, int state_dim, const double* m, const double* s, double* muR, double* sR);
/* Particle rollout through the learned dynamics (extension): P sampled trajectories of H steps, all on
 * the device, to hold against the Gaussians pilco_rollout propagates.  One step of particle p, D = E + U:
 *   u = the policy's deterministic action at x = controller.compute_action(x, 0)[0] (pilco/models/pilco.py:115):
 *       LINEAR  max_action * sin(x W^T + b);   RBF  max_action * exp(-0.5e-6) * sin(sum_i beta_ui k_u(x, c_i)), the policy GP
 *       of PILCO_SLOT_POLICY (exp(-0.5e-6): the reference's S - diag(variance - 1e-6) at s = 0, controllers.py:117);
 *       NONE  no control, D = E;  squash = 0: the argument of the sine itself
 *   (mu_e, v_e) = the posterior of output e at [x, u] -- what pilco_gp_predict_points returns (exact GP or FITC on the
 *       slot's shared Z); at s = 0 the moment matching of mgpr.py:91-149 gives exactly this Gaussian
 *   x'_e = x_e + mu_e + sqrt(max(v_e [+ likelihood variance_e], 0)) * eps[t][p][e]     (the GP predicts differences,
 *       pilco.py:138-153)
 * x0 (P,E) initial particles.  eps (H,P,E) standard-normal draws, or NULL: generated on the device from seed (Philox4x32-10
 * and Box-Muller, csrc/philox_normal.h: a draw depends on (seed, t, p, e) only).  observation_noise 0: latent variance
 * (what moment matching propagates); 1: + likelihood variance.
 * mean (H+1,E), cov (H+1,E,E): empirical moments of the particles after every step, row 0 = x0; the covariance divides by
 * P (P = 1 gives zeros).  reward_steps (H, may be NULL): mean over the particles of the reward terms at zero covariance --
 * exponential exp(-0.5 (x-t) W (x-t)^T), linear W.x, combined by coef -- of the PRE-step states 0..H-1 (the convention of
 * pilco_rollout).  particles (H+1,P,E) and eps_out (H,P,E), the draws actually used: may be NULL.
 * A particle's trajectory depends on its own x0 row and its own draws only: the same bits alone or in any batch.  The sums
 * behind mean, cov and reward_steps run in a fixed order (no floating-point atomics): particles in index order inside blocks
 * of 128, the blocks in index order; the same particles give the same bits.  All H steps are enqueued in one pass -- one upload,
 * one download, one synchronisation; the particles are chunked like pilco_gp_predict_points: bounded memory for any P.
 * Needs the dynamics slot's own factorisation (factorises if it is not current).  PILCO_E_STATE on a sharded or multi-rank
 * context, after pilco_gp_set_factors, or for an RBF policy whose slot is not factorised; PILCO_E_SHAPE for P <= 0, H < 0, a
 * null x0 / mean / cov or a policy whose dimensions do not match the slot. */
int pilco_rollout_particles(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                            const double* x0, int P, int H, const double* eps, unsigned long long seed, int observation_noise,
                            double* mean, double* cov, double* reward_steps, double* particles, double* eps_out);
/* Constraint events on the particles (extension; docs/particles.md): an event is a box over a few state coordinates, or the
 * complement of one.  inside(x): every clause holds, low <= x[dim] && x[dim] <= high (closed intervals; -INFINITY /
 * +INFINITY: no bound on that side).  hit(x) = complement ? !inside(x) : inside(x).  A NaN coordinate fails its clause:
 * inside is false and hit equals complement.  The predicate itself is csrc/particle_events.h (host and device).
 * Safe-PILCO's RiskOfCollision(state_dim, low, high) is two clauses, on dims 0 and 2; SingleConstraint(dim, high, low,
 * inside) is one clause with complement = !inside. */
#define PILCO_MAX_EVENTS 8
#define PILCO_MAX_EVENT_CLAUSES 4
typedef struct pilco_event_clause { int dim; double low, high; } pilco_event_clause;   /* -INFINITY / +INFINITY: no bound on that side */
typedef struct pilco_event { int n_clauses; int complement; pilco_event_clause clause[PILCO_MAX_EVENT_CLAUSES]; } pilco_event;
/* pilco_rollout_particles with events counted on the device: the same arguments in the same order, the same launches and
 * the same output bits, and behind the statistics of every state t = 0..H (row 0 = x0) two counting launches over all
 * particles of the step.  counts (H+1, n_events): the number of particles with hit at state t.  first_hit (P, n_events),
 * may be NULL: the smallest t in 0..H at which particle p hits event k, or -1.  Integer results: blocks of 128 particles
 * count by wave ballot, the blocks' counts are added in block order; no atomics.  Both arrive with the call's one download.
 * n_events = 0 is pilco_rollout_particles itself.  PILCO_E_SHAPE, before any launch or upload, for n_events outside
 * 0..PILCO_MAX_EVENTS, n_events > 0 with a null events or counts, n_clauses outside 1..PILCO_MAX_EVENT_CLAUSES, a dim
 * outside [0, E), a NaN bound or low > high; and for everything pilco_rollout_particles refuses. */
int pilco_rollout_particles_events(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                   const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                   int observation_noise, double* mean, double* cov, double* reward_steps, double* particles,
                                   double* eps_out, const pilco_event* events, int n_events, long long* counts, int* first_hit);
/* Value and pathwise gradient of the particle return (extension; docs/particle_gradients.md).  With x0 and the draws fixed
 * (eps given, or the Philox stream of seed exactly as pilco_rollout_particles generates it), J = sum_t (1/P) sum_p r(x_t^p)
 * over the PRE-step states t = 0..H-1 is a smooth function of the controller parameters.  reward = J, the sum in step order of
 * reward_steps (H, may be NULL), which has the bits of pilco_rollout_particles on the same inputs.  dW (U,E), db (U): dJ / d
 * (W, b) of a LinearController; ignored (may be NULL) for PILCO_POLICY_NONE.  dreturn_dx0 (P,E), may be NULL: row p is the
 * gradient of particle p's OWN return sum_t r(x_t^p) w.r.t. its x0 row (not divided by P); it has the same bits alone or in any
 * batch.  The derivative through the clamp sqrt(max(v, 0)) is 0 where v <= 0.
 * The forward pass stores one (E, D) step matrix per particle and step t < H-1; above a budget (1 GiB; the environment's
 * PILCO_PARTICLE_GRAD_BUDGET, in doubles, read at every call) the particles run in groups of a multiple of 128, one after the
 * other.  The parameter sums run in a fixed order without floating-point atomics (particles in index order inside blocks of
 * 128 per step, the steps t = H-2..0 added to the block's cell, the cells in block order, one division by P): neither the
 * chunks nor the groups change a bit of any output.  One upload; one download and synchronisation per group and one at the end.
 * Refuses what pilco_rollout_particles refuses, a null reward, a policy kind other than NONE / LINEAR, and a null dW or db for
 * a LinearController -- all before any launch or upload, the outputs untouched. */
int pilco_rollout_particles_grad(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                 const double* x0, int P, int H, const double* eps, unsigned long long seed, int observation_noise,
                                 double* reward, double* reward_steps, double* dW, double* db, double* dreturn_dx0);
/* The same for an RbfController whose GP lives in PILCO_SLOT_POLICY: gradients w.r.t. the centres Xp (bf,E), the targets Yp
 * (bf,U) and the lengthscales lsp (U,E); the caller passes the host copies of the parameters it uploaded, as for
 * pilco_rollout_grad_rbf (noisep (U)).  Also refuses null Xp / Yp / lsp / noisep / dX / dY / dls, a bf that is not the policy
 * slot's number of points, and (PILCO_E_NOT_PD) a singular K + noise I. */
int pilco_rollout_particles_grad_rbf(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                     const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                     int observation_noise, const double* Xp, const double* Yp, const double* lsp,
                                     const double* noisep, int bf, double* reward, double* reward_steps, double* dX, double* dY,
                                     double* dls, double* dreturn_dx0);
/* A neural-network policy for the particle entry points (extension; docs/particle_mlp.md): one hidden layer of `hidden` tanh
 * units, x the state (E), j < hidden, k < U,
 *   a_j = b1_j + sum_e W1_je x_e,   h_j = tanh(a_j),   s_k = b2_k + sum_j W2_kj h_j,   u_k = squash ? max_action_k sin(s_k) : s_k
 * (the squash of the LinearController on particles: zero covariance, no exp(-0.5e-6) factor).  Every kernel evaluates the sums
 * in one order: a_j by fma over e ascending from 0, then + b1_j; s_k by fma over j ascending from 0, then + b2_k.
 * pilco_set_policy_mlp copies W1 (hidden,E), b1 (hidden), W2 (U,hidden), b2 (U) into the context on the host (no device call);
 * a pilco_policy of kind PILCO_POLICY_MLP (W, b NULL; max_action, squash, state_dim, control_dim as for the linear kind) then
 * acts with them in pilco_rollout_particles, _events, _fn, _cond and pilco_debug_particle_actions: the parameters travel in the
 * call's one parameter upload.  PILCO_E_SHAPE for hidden outside 1..PILCO_MAX_MLP_HIDDEN, state_dim or control_dim < 1 or
 * state_dim + control_dim > 32, or a null pointer: the context keeps what it had.  A particle entry point refuses kind 3 with
 * PILCO_E_STATE when no network is set and with PILCO_E_SHAPE when the network's dimensions are not the dynamics slot's, before
 * any launch or upload.  The moment-matching entry points (pilco_rollout*, pilco_propagate, pilco_policy_action) refuse kind 3:
 * a network has no closed-form action moments. */
#define PILCO_MAX_MLP_HIDDEN 256
int pilco_set_policy_mlp(pilco_ctx* ctx, int state_dim, int control_dim, int hidden, const double* W1, const double* b1,
                         const double* W2, const double* b2);
/* pilco_rollout_particles_grad for the network of pilco_set_policy_mlp: dW1 (hidden,E), db1 (hidden), dW2 (U,hidden), db2 (U)
 * in place of dW, db; everything else (reward, reward_steps, dreturn_dx0, eps, seed, observation_noise, the order of the sums,
 * the groups) as there.  With ds_k = g_u[k] (squash ? max_action_k cos(s_k) : 1) and delta_j = (1 - h_j^2) sum_k W2_kj ds_k:
 * dW1_je = sum_p delta_pj x_pe, db1_j = sum_p delta_pj, dW2_kj = sum_p ds_pk h_pj, db2_k = sum_p ds_pk, over P.  Refuses what
 * pilco_rollout_particles_grad refuses, a policy kind other than MLP, and a null dW1, db1, dW2 or db2 -- all before any launch
 * or upload, the outputs untouched.  pilco_rollout_particles_grad / _grad_rbf refuse kind 3. */
int pilco_rollout_particles_grad_mlp(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                     const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                     int observation_noise, double* reward, double* reward_steps, double* dW1, double* db1,
                                     double* dW2, double* db2, double* dreturn_dx0);
/* Particle rollout on posterior FUNCTION samples (extension; docs/particle_functions.md).  pilco_rollout_particles moves a
 * particle by an independent marginal draw per step; here particle p draws ONE dynamics function f_p from the GP posterior
 * (pathwise conditioning on a random-Fourier-feature prior with L features, exact GP only) and rolls it out
 * deterministically: with xt = [x, u],
 *   phi_el(xt) = sqrt(2 var_e / L) cos(omega_el . xt + b_el),   omega_eld = z_eld / lengthscale_ed,  b_el = 2 pi u
 *   r_pe = y_e - Phi_e(X) w_pe - sqrt(noise_e) xi_pe,   v_pe = iK_e r_pe   (iK: the slot's own (K + noise I)^-1)
 *   f_pe(xt) = sum_l w_pel phi_el(xt) + sum_i k_e(xt, X_i) v_pei,   x'_e = x_e + f_pe(xt) [+ sqrt(noise_e) eps[t][p][e]]
 * Every argument before draws means what it means in pilco_rollout_particles_events; eps and eps_out are read and written
 * only with observation_noise.  draws: L and either all four of omega (E,L,D), phase (E,L), w (P,E,L), xi (P,E,N) or none of
 * them (generated from seed, csrc/philox_normal.h, domains 1..4; the features are shared by all particles).  draws_out (may
 * be NULL, each member may be NULL): the draws used and v (P,E,N); feeding them back reproduces every output bitwise.
 * A particle's trajectory depends on its own x0 row and its own (w_p, xi_p) only: the same bits alone or in any batch.
 * All particles' v are live at every step: the call holds E Ppad (Lpad + 2 npad) doubles (Ppad, Lpad, npad: P, L, N rounded
 * up to 64) and is refused above a budget of 2^29 doubles (the environment's PILCO_PARTICLE_FN_BUDGET, in doubles, read at
 * every call) with the largest P that fits in the message.  Refuses, before any launch or upload and with nothing written,
 * what pilco_rollout_particles_events refuses, a sparse slot (PILCO_E_STATE), a null draws, L outside 1..4096 and some but
 * not all of the four draws given (PILCO_E_SHAPE). */
#define PILCO_MAX_FN_FEATURES 4096
typedef struct pilco_function_draws { int L; const double *omega, *phase, *w, *xi; } pilco_function_draws;
typedef struct pilco_function_draws_out { double *omega, *phase, *w, *xi, *v; } pilco_function_draws_out;
int pilco_rollout_particles_fn(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                               const double* x0, int P, int H, const double* eps, unsigned long long seed, int observation_noise,
                               double* mean, double* cov, double* reward_steps, double* particles, double* eps_out,
                               const pilco_event* events, int n_events, long long* counts, int* first_hit,
                               const pilco_function_draws* draws, const pilco_function_draws_out* draws_out);
/* Value and pathwise gradient of the FUNCTION-sample particle return (extension; docs/particle_fn_gradients.md).  With x0,
 * the draws and (observation_noise) eps fixed, particle p follows one function f_p, and J = sum_t (1/P) sum_p r(x_t^p) over the
 * pre-step states t = 0..H-1 is a plain deterministic function of the controller parameters: the step matrix is
 *   A_t[e][d] = [e == d] + d f_pe / d z_d,   z = [x, u],
 *   d f_pe / d z_d = -sqrt(2 var_e / L) sum_l w_pel sin(omega_el . z + b_el) omega_eld - var_e sum_i k_i v_pei (z_d - X_id) / l_ed^2
 * (no clamp, no variance derivative; additive observation noise does not enter it), and the reverse sweep, the policy
 * adjoints, the rewards' gradients and the parameter sums are those of pilco_rollout_particles_grad.  draws / draws_out: as
 * pilco_rollout_particles_fn (draws_out returns the draws used, so a repeat or a finite-difference call sees the same
 * functions); eps (H,P,E) is read only with observation_noise (NULL: the stream of seed).  reward = J, the sum in step order of
 * reward_steps (H, may be NULL), which has the bits of pilco_rollout_particles_fn on the same inputs and draws.  dW, db,
 * dreturn_dx0: as pilco_rollout_particles_grad.  H = 0: value 0, zero gradients; H = 1: zero policy gradients, dreturn_dx0 =
 * grad r(x0).
 * The set-up of pilco_rollout_particles_fn runs once per call and its budget (PILCO_PARTICLE_FN_BUDGET) refuses as there; the
 * stored matrices, (H-1) P E D doubles, obey PILCO_PARTICLE_GRAD_BUDGET: above it the particles run in groups of a multiple of
 * 128, each forward then reverse over its own columns of the weights.  Every sum has a fixed order without floating-point
 * atomics: neither the groups nor the batch change a bit of any output.  One upload; one download and synchronisation per
 * group (only with dreturn_dx0) and one at the end.  Refuses what pilco_rollout_particles_grad refuses and what
 * pilco_rollout_particles_fn refuses about the slot, the draws and the budget -- all before any launch or upload, the outputs
 * untouched. */
int pilco_rollout_particles_fn_grad(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                    const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                    int observation_noise, const pilco_function_draws* draws,
                                    const pilco_function_draws_out* draws_out, double* reward, double* reward_steps, double* dW,
                                    double* db, double* dreturn_dx0);
/* The same for an RbfController whose GP lives in PILCO_SLOT_POLICY; the arguments after draws_out and the further refusals
 * are those of pilco_rollout_particles_grad_rbf. */
int pilco_rollout_particles_fn_grad_rbf(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                        const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                        int observation_noise, const pilco_function_draws* draws,
                                        const pilco_function_draws_out* draws_out, const double* Xp, const double* Yp,
                                        const double* lsp, const double* noisep, int bf, double* reward, double* reward_steps,
                                        double* dX, double* dY, double* dls, double* dreturn_dx0);
/* The same for the network of pilco_set_policy_mlp; the gradient arguments are those of pilco_rollout_particles_grad_mlp. */
int pilco_rollout_particles_fn_grad_mlp(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                        const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                        int observation_noise, const pilco_function_draws* draws,
                                        const pilco_function_draws_out* draws_out, double* reward, double* reward_steps,
                                        double* dW1, double* db1, double* dW2, double* db2, double* dreturn_dx0);
/* Particle rollout CONDITIONED ON ITS OWN PATH (extension; docs/particle_conditioned.md): exact and consistent along a
 * trajectory, for the exact GP and for FITC on the slot's shared inducing inputs.  The increments f(xt_0), .., f(xt_{H-1}) of a
 * particle (xt = [x, u]) are jointly Gaussian under the posterior; step t is drawn conditioned on the particle's own earlier
 * visited points.  Per particle and output e, with the rows w of pilco_gp_predict_points_cov:
 *   c_ts = k_e(xt_t, xt_s) - w_t . w_s  (FITC: - w0_t . w0_s + w1_t . w1_s);   Lam Lam^T = C + jitter * variance_e * I by rows:
 *   l_s = (c_ts - sum_{r<s} l_r Lam_sr) / Lam_ss,  d = c_tt + jitter * variance_e - sum_{s<t} l_s^2,  Lam_tt = sqrt(d)
 *   x'_e = x_e + mu_t + sum_{s<t} l_s z_s + Lam_tt z_t  [+ sqrt(likelihood variance_e) zeta_t  with observation_noise]
 * mu_t has the bits of pilco_gp_predict_points; z_s = eps[s][p][e] is the step stream of pilco_rollout_particles (the same seed
 * gives the same first step up to the jitter); zeta is a second, independent stream (Philox domain 6, counter {p, t, j, 6}) and
 * never enters the conditioning.  Every argument up to first_hit means what it means in pilco_rollout_particles_events.
 * jitter: relative to the kernel variance, finite and >= 0 (1e-8 is the binding's default).  eps_obs (H,P,E), may be NULL: the
 * caller's zeta, read only with observation_noise.  out (may be NULL, each member may be NULL): eps_obs (H,P,E), the zeta
 * used, written only with observation_noise; path_cov and path_factor (P,E,H,H): c_ts (without jitter) and Lam in the lower
 * triangle, zero above it.  A trajectory depends on its own x0 row and draws only: the same bits alone, in any batch or group.
 * The call holds H nops E npad + E H (H+1) / 2 + H D + E npad + 2 E doubles per particle (nops: 1 exact, 2 FITC; the factor twice
 * with path_cov) and runs in groups of a multiple of 64 particles within a budget of 2^29 doubles (the environment's
 * PILCO_PARTICLE_COND_BUDGET, in doubles, read at every call); the statistics and events run after the last group over all
 * particles, so grouping changes no bit.  Refuses, before any launch or upload and with nothing written, what
 * pilco_rollout_particles_events refuses, H > PILCO_MAX_COND_STEPS, a jitter that is negative or not finite, nops * npad > 8192
 * and a footprint over the budget for a group of 64 (the message names the largest H that fits).  PILCO_E_NOT_PD when a pivot
 * d is not positive (NaN included): the message names particle, output and step (the earliest such step, there the lowest
 * particle, then output), and nothing is written. */
#define PILCO_MAX_COND_STEPS 128
typedef struct pilco_cond_out { double *eps_obs, *path_cov, *path_factor; } pilco_cond_out;   /* each may be NULL */
int pilco_rollout_particles_cond(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                 const double* x0, int P, int H, const double* eps, unsigned long long seed, int observation_noise,
                                 double* mean, double* cov, double* reward_steps, double* particles, double* eps_out,
                                 const pilco_event* events, int n_events, long long* counts, int* first_hit,
                                 double jitter, const double* eps_obs, const pilco_cond_out* out);

/* ------------------------------------------------------------------ reverse mode
 * The reference differentiates training_loss with TensorFlow's autodiff (pilco/models/pilco.py:85-90);
 * here the adjoint of the moment-matching step is hand-derived.
 * pilco_gp_predict_vjp: cotangents Mbar (1,E), Sbar (E,E), Vbar (D,E) of pilco_gp_predict's outputs ->
 * mbar (1,D), sbar (D,D, symmetric) at the input (m, s).  Single rank, D <= 32. */
int pilco_gp_predict_vjp(pilco_ctx* ctx, int slot, const double* m, const double* s, const double* Mbar,
                         const double* Sbar, const double* Vbar, double* mbar, double* sbar);
/* Cotangent seeds for objectives beyond the additive reward (SafePILCO's multiplicative risk term,
 * safe_pilco_extension/safe_pilco.py:29-50; any function of the state trajectory): after the forward pass the library
 * calls seed_fn(user, H, E, traj, seeds) with traj [H+1][E + E*E] (m_t | s_t, t = 0..H; state t < H is the
 * pre-propagation state the reward of step t sees) and seeds [H+1][E + E*E] zero-filled; the callback writes
 * d objective / d (m_t, s_t) and the reverse sweep adds them where the reward's own cotangents enter.  *reward is the
 * additive reward only: the caller adds its own term.  What TensorFlow's reverse mode through training_loss gives the
 * reference for whatever predict() returns (pilco/models/pilco.py:47-50, 85-90). */
typedef void (*pilco_seed_fn)(void* user, int H, int E, const double* traj, double* seeds);
int pilco_rollout_grad_seeded(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                              const double* m0, const double* S0, int H, pilco_seed_fn seed_fn, void* seed_user, double* reward,
                              double* dW, double* db);
int pilco_rollout_grad_rbf_seeded(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                  const double* m0, const double* S0, int H, const double* Xp, const double* Yp, const double* lsp,
                                  const double* noisep, int bf, pilco_seed_fn seed_fn, void* seed_user, double* reward, double* dX,
                                  double* dY, double* dls);
/* Value and gradient of the rollout reward w.r.t. a squashed LinearController's parameters, dW (U,E) and db (U):
 * training_loss + TensorFlow reverse mode in the reference (pilco/models/pilco.py:47-50,85-90).  Forward rollout
 * with a tape, then the reverse sweep with the moment-matching adjoint of every step on the device and the O(D^3)
 * links (propagate, joint Gaussian, controller + squash, rewards) in native host code. */
int pilco_rollout_grad(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                       const double* m0, const double* S0, int H, double* reward, double* dW, double* db);
/* The same for an RbfController (policy GP in PILCO_SLOT_POLICY, pilco/controllers.py:80-129): gradients w.r.t. the
 * centres dX (bf,E), the targets dY (bf,U) and the lengthscales dls (U,E).  Xp, Yp, lsp, noisep (U): host copies of the
 * policy parameters that were uploaded with pilco_gp_set_data / pilco_gp_set_hyp (noise = FakeGPR likelihood variance). */
int pilco_rollout_grad_rbf(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                           const double* m0, const double* S0, int H, const double* Xp, const double* Yp, const double* lsp,
                           const double* noisep, int bf, double* reward, double* dX, double* dY, double* dls);
/* B value-and-gradient rollouts of ONE dynamics model in flight together -- the restarts of PILCO.optimize_policy
 * (pilco/models/pilco.py:94-107 runs them one after the other; each restart is an L-BFGS-B walk of its own, so the evaluations
 * of different restarts are independent).  Lanes as in pilco_rollout_batch; every lane's result is BIT-IDENTICAL to its solo
 * pilco_rollout_grad call.  LinearController lanes: policies[i].W / .b; m0 (B,E), S0 (B,E,E); reward (B), dW (B,U,E), db (B,U). */
int pilco_rollout_grad_batch(pilco_ctx* ctx, int B, const pilco_policy* policies, const pilco_reward_term* rewards, int n_rewards,
                             const double* m0, const double* S0, int H, double* reward, double* dW, double* db);
/* RbfController lanes: lane i's policy GP -- centres Xp (B,bf,E), targets Yp (B,bf,U), lengthscales lsp (B,U,E), likelihood
 * variances noisep (B,U), unit signal variance (pilco/controllers.py:92-93) -- is uploaded to and factorised in
 * PILCO_SLOT_POLICY of lane i's context BY THIS CALL, lane 0 = this context included: the caller's policy slot holds lane 0's
 * controller afterwards.  reward (B), dX (B,bf,E), dY (B,bf,U), dls (B,U,E); bit-identical to the solo pilco_rollout_grad_rbf. */
int pilco_rollout_grad_rbf_batch(pilco_ctx* ctx, int B, const pilco_policy* policies, const pilco_reward_term* rewards, int n_rewards,
                                 const double* m0, const double* S0, int H, const double* Xp, const double* Yp, const double* lsp,
                                 const double* noisep, int bf, double* reward, double* dX, double* dY, double* dls);
/* ... with an objective beyond the additive reward (Safe-PILCO's risk term, host-evaluated reward terms), as
 * pilco_rollout_grad_seeded: seed_fn is called once per lane, in lane order, with seed_users[i] (seed_users may be NULL), when
 * lane i's trajectory has arrived and before its reverse sweep; reward[i] is lane i's additive reward alone. */
int pilco_rollout_grad_batch_seeded(pilco_ctx* ctx, int B, const pilco_policy* policies, const pilco_reward_term* rewards, int n_rewards,
                                    const double* m0, const double* S0, int H, pilco_seed_fn seed_fn, void* const* seed_users,
                                    double* reward, double* dW, double* db);
int pilco_rollout_grad_rbf_batch_seeded(pilco_ctx* ctx, int B, const pilco_policy* policies, const pilco_reward_term* rewards, int n_rewards,
                                        const double* m0, const double* S0, int H, const double* Xp, const double* Yp, const double* lsp,
                                        const double* noisep, int bf, pilco_seed_fn seed_fn, void* const* seed_users, double* reward,
                                        double* dX, double* dY, double* dls);

/* (timing and introspection entry points -- HIP-event timers, in-kernel phase stamps, raw work buffers, the stream-K split --
 * are developer aids of the same library, declared in include/pilco_hip_dev.h: not part of the boundary a binding needs.) */

/* ------------------------------------------------------------------ multi-GPU
 * One process per GPU.  The P = E(E+1)/2 output pairs (and with them the
 * outputs' factorisations) are dealt round-robin over the ranks; one
 * ncclAllGather (RCCL over xGMI) per horizon step reassembles (M, S, V).
 * id: 128 opaque bytes produced on rank 0 and broadcast by the host launcher. */
#define PILCO_COMM_ID_BYTES 128
int pilco_comm_unique_id(void* id128);
int pilco_comm_init(pilco_ctx* ctx, const void* id128, int rank, int nranks);
/* sharding without a communicator: the caller moves the bytes (host fake
 * all-gather for tests; gloo fallback).  Pairs are dealt round-robin in the order (0,0),(1,1),..,(E-1,E-1),(1,0),(2,0),(2,1),..;
 * output a belongs to the owner of (a,a)  (the plan's introspection functions: include/pilco_hip_dev.h). */
int pilco_shard_set(pilco_ctx* ctx, int rank, int nranks);
/* One sharded moment-matching step with the exchange done by the caller: shard_pack runs this
 * rank's pairs and returns its SEG doubles; after an all-gather by any transport, shard_finish
 * assembles (M, S, V) from the [nranks][SEG] buffer.  pilco_gp_predict / pilco_rollout do the
 * same with ncclAllGather when a communicator is attached. */
int pilco_gp_shard_pack(pilco_ctx* ctx, int slot, const double* m, const double* s, double* segment);
int pilco_gp_shard_finish(pilco_ctx* ctx, int slot, const double* gathered, double* M, double* S, double* V);
/* Sharded factorisation: with nranks > 1 pilco_gp_factorize computes and stores K / L^-1 / iK only for the outputs this
 * rank owns (a = rank, rank + nranks, ...; memory and work / nranks, no communication) and then needs every rank's beta
 * rows: one ncclAllGather per MODEL when a communicator is attached, or -- contexts of one process -- this call, after
 * all of them have factorised. */
int pilco_group_sync_model(pilco_ctx** ctxs, int n, int slot);
/* The same beta exchange over any host transport (ranks in different processes, no communicator): pilco_gp_beta_rows
 * gives the block shape (elcap = ceil(E / nranks) rows of npad doubles per rank), every rank exports the rows it
 * computed, the caller all-gathers the blocks in rank order, every rank imports [nranks][elcap][npad]. */
int pilco_gp_beta_rows(pilco_ctx* ctx, int slot, int* elcap, int* npad);
int pilco_gp_beta_export(pilco_ctx* ctx, int slot, double* own_rows);
int pilco_gp_beta_import(pilco_ctx* ctx, int slot, const double* all_rows);
/* The whole sharded rollout over n contexts of ONE process (context i = rank i of n; several contexts may share a GPU):
 * every context runs pilco_rollout on its own host thread and the per-step exchange is done with peer copies between
 * host barriers instead of ncclAllGather -- the same launch sequence as the RCCL path, so the multi-rank rollout can be
 * validated without a multi-GPU node (host-synchronised per step: a test vehicle, not a fast path).
 * Outputs are rank 0's; *mismatch (may be NULL) = 1 if another rank finished with a different bit pattern. */
int pilco_rollout_group(pilco_ctx** ctxs, int n, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                        const double* m0, const double* S0, int H, double* mH, double* SH, double* reward, double* traj,
                        int* mismatch);
/* Value and gradient of ONE sharded rollout (pilco_rollout_grad, LinearController) over n contexts of this process, as
 * pilco_rollout_group does the forward rollout: every rank sweeps its own pairs, the per-pair Jacobian records are
 * all-gathered once after the horizon (between processes pilco_rollout_grad does that itself with ncclAllGather when a
 * communicator is attached), every rank runs the same host reverse sweep on the same records.  reward [n], dW [n][U*E],
 * db [n][U]: every rank's results (bit-identical to one another). */
int pilco_rollout_grad_group(pilco_ctx** ctxs, int n, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                             const double* m0, const double* S0, int H, double* reward, double* dW, double* db);
/* The same for an RbfController (pilco_rollout_grad_rbf on every context; pilco/controllers.py:80-129).  The policy GP is not
 * sharded -- every rank holds all of it in PILCO_SLOT_POLICY and evaluates it inside its link kernel (inline policy: at most
 * 256 basis functions).  reward [n], dX [n][bf*E], dY [n][bf*U], dls [n][U*E]: every rank's results, bit-identical to one
 * another and to the single-rank pilco_rollout_grad_rbf (the split of every pair's sums does not depend on the rank count). */
int pilco_rollout_grad_rbf_group(pilco_ctx** ctxs, int n, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                 const double* m0, const double* S0, int H, const double* Xp, const double* Yp, const double* lsp,
                                 const double* noisep, int bf, double* reward, double* dX, double* dY, double* dls);
/* Peer exchange: the per-step all-gather without a collective call.  Every rank owns an exchange area in its GPU's
 * memory; after its pair kernel a rank stores its segment straight into EVERY rank's area (over xGMI between GPUs) and
 * raises its flag there; the next step's head waits for the W flags of that exchange and reads the segments from its
 * own memory.  No host involvement per step, no RCCL launch (~20 us) on the critical path; the whole sharded rollout is
 * captured in one hipGraph.  Used by pilco_rollout whenever it is attached (linear / no policy; otherwise the RCCL path).
 *   ranks in different processes: pilco_peer_export on every rank (64 opaque bytes = a hipIpcMemHandle_t), all-gather the
 *   handles by any host transport, pilco_peer_attach(handles[nranks][64]).  share_gpu != 0 when ranks share a GPU
 *   (oversubscribed tests): the flag wait then runs as a one-workgroup launch of its own so that waiting kernels cannot
 *   keep the awaited ones off the machine.
 *   contexts of one process: pilco_group_peer_attach(ctxs, n).  When they share a GPU, pilco_rollout_group enqueues the
 *   ranks' launches step by step in lockstep and without a graph: their streams may share hardware queues, and every
 *   push of a step is then in the queues before any wait for it.
 * A wait that gives up (~2 s) makes pilco_rollout return PILCO_E_STATE instead of hanging.  All ranks must make the same
 * sequence of pilco_rollout calls.  pilco_shard_set / pilco_comm_init detach. */
#define PILCO_PEER_HANDLE_BYTES 64
int pilco_peer_export(pilco_ctx* ctx, void* handle64);
int pilco_peer_attach(pilco_ctx* ctx, const void* handles, int share_gpu);
int pilco_group_peer_attach(pilco_ctx** ctxs, int n);
int pilco_peer_detach(pilco_ctx* ctx);
int pilco_comm_rank(const pilco_ctx* ctx);
int pilco_comm_size(const pilco_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* PILCO_HIP_H */
