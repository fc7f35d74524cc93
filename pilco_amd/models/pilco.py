"""PILCO rollout driver with the reference's interface
(/root/reference/pilco/models/pilco.py:15-160).  ``predict`` runs the whole
H-step moment-matching rollout on the device in one call (pilco_rollout)."""
from __future__ import annotations

import time

import numpy as np

from .. import _lib, controllers, rewards
from ..params import parameters_of, set_trainable
from .mgpr import MGPR
from .smgpr import SMGPR


class ParticleTrajectories:
    """What PILCO.sample_trajectories returns: mean (n+1, E) and cov (n+1, E, E) of the particles after every step (row 0:
    the initial particles), reward (1, 1) = reward_steps.sum() -- comparable with predict(...)[2] --, reward_steps (n,),
    particles (n+1, P, E) or None, eps (n, P, E): the standard-normal draws used.  With events: event_counts (n+1, K), the
    number of particles that hit event k at state t; event_prob = event_counts / P; first_hit (P, K), the first such t of
    every particle or -1.  None without events.  function_draws: with dynamics="function" and return_particles=True the
    dict of omega (E, L, D), phase (E, L), w (P, E, L), xi (P, E, N), v (P, E, N) the call used (docs/particle_functions.md);
    else None.  eps_obs (n, P, E), path_cov and path_factor (P, E, n, n): with dynamics="conditioned" and
    return_particles=True the observation-noise draws used (None without observation_noise), the path covariance c_ts and
    its factor, lower triangles (docs/particle_conditioned.md); else None."""

    def __init__(self, mean, cov, reward_steps, particles, eps, event_counts=None, first_hit=None, function_draws=None, *,
                 eps_obs=None, path_cov=None, path_factor=None):
        self.mean, self.cov, self.reward_steps, self.particles, self.eps = mean, cov, reward_steps, particles, eps
        self.function_draws = function_draws
        self.eps_obs, self.path_cov, self.path_factor = eps_obs, path_cov, path_factor
        self.reward = np.asarray(reward_steps, np.float64).sum().reshape(1, 1)
        self.event_counts, self.first_hit = event_counts, first_hit
        self.event_prob = None if event_counts is None else event_counts / float(first_hit.shape[0])

    def __repr__(self):
        return "ParticleTrajectories(steps=%d, state_dim=%d, reward=%.6g)" % (self.mean.shape[0] - 1, self.mean.shape[1], self.reward[0, 0])


class Linearization:
    """What PILCO.linearize returns: the local model x' ~ x_next + A (x - x0) + B (u - u0) of the learned dynamics at
    (x0, u0).  x_next (Nt, E) = x + posterior mean, var (Nt, E) its latent variance, A (Nt, E, E) = I + d mean / d x,
    B (Nt, E, U) = d mean / d u, dvar_dx (Nt, E, E), dvar_du (Nt, E, U), u (Nt, U); K (Nt, U, E), the controller's
    action Jacobian, and A_cl = A + B K where the action was the controller's own, else None.  A single state: the same
    fields without the leading axis."""
    fields = ("x_next", "var", "A", "B", "dvar_dx", "dvar_du", "u", "K", "A_cl")

    def __init__(self, **kw):
        for f in self.fields:
            setattr(self, f, kw[f])

    def __repr__(self):
        return "Linearization(A%s, B%s%s)" % (np.shape(self.A), np.shape(self.B), "" if self.K is None else ", closed loop")


class PILCO:
    def __init__(self, data, num_induced_points=None, horizon=30, controller=None,
                 reward=None, m_init=None, S_init=None, name=None, ctx=None):
        self.name = name
        self._ctx = ctx   # None: decided on first use (the ctx property) -- constructing a model touches no device
        if num_induced_points is None:
            self.mgpr = MGPR(data, ctx=ctx)
        else:
            self.mgpr = SMGPR(data, num_induced_points, ctx=ctx)
        self.state_dim = data[1].shape[1]
        self.control_dim = data[0].shape[1] - data[1].shape[1]
        self.horizon = horizon
        if controller is None:
            self.controller = (controllers.LinearController(self.state_dim, self.control_dim, ctx=ctx)
                               if self.control_dim > 0 else None)
        else:
            self.controller = controller
        self.reward = rewards.ExponentialReward(self.state_dim) if reward is None else reward
        import weakref
        for comp in (self.mgpr, self.controller, getattr(self.controller, "_gp", None), self.reward):
            if comp is not None and getattr(comp, "_ctx", None) is None:   # components without a context will ask this object for its
                ref = getattr(comp, "_ctx_owner", None)
                if ref is not None and ref() is not None:
                    continue   # a component shared with another live PILCO object stays with it (and this object joins: ctx below)
                try:
                    comp._ctx_owner = weakref.ref(self)
                except AttributeError:
                    pass
        if m_init is None or S_init is None:
            # pilco.py:37-41: first state of the data set, 0.1 * I
            self.m_init = np.asarray(data[0])[0:1, 0:self.state_dim]
            self.S_init = np.diag(np.ones(self.state_dim) * 0.1)
        else:
            self.m_init = m_init
            self.S_init = S_init
        self.optimizer = None

    @property
    def ctx(self):
        if self._ctx is None:
            # a component that already lives on a context decides; otherwise a context of this object's own: the default one
            # for the first live PILCO object, a pooled one for every further (_lib.context_for)
            # (only the components that hold device slots decide -- the models, the controller and its GP; a stateless
            # reward object reused by several PILCO objects must not pull them all onto one context)
            comps = [c for c in (self.mgpr, self.controller, getattr(self.controller, "_gp", None)) if c is not None]
            for comp in comps:
                if getattr(comp, "_ctx", None) is not None:
                    self._ctx = comp._ctx
                    _lib.context_adopted(self._ctx, self)   # ... and this object is now that context's holder in the pool
                    break
            if self._ctx is None:
                for comp in comps:   # a component that belongs to another live PILCO object (a shared controller): one context for both
                    ref = getattr(comp, "_ctx_owner", None)
                    other = ref() if ref is not None else None
                    if other is not None and other is not self:
                        self._ctx = other.ctx
                        break
            if self._ctx is None:
                self._ctx = _lib.context_for(self)
        return self._ctx

    def _policy_spec(self):
        if self.control_dim == 0 or self.controller is None:
            return dict(kind=_lib.POLICY_NONE, state_dim=self.state_dim, control_dim=0)
        return self.controller.policy_spec(True)

    # -- reward terms: on the device (exponential / linear) and, for anything else, on the host along the trajectory
    def _reward_terms(self):
        terms = self.reward.terms() if hasattr(self.reward, "terms") else []
        return terms or [dict(kind=_lib.REWARD_LINEAR, coef=0.0, W=np.zeros(self.state_dim))]    # the C ABI wants one term

    def _host_reward_terms(self):
        r = getattr(self, "reward", None)
        if r is None:
            return []
        if hasattr(r, "terms"):
            return r.host_terms() if hasattr(r, "host_terms") else []
        return [(1.0, r)]                       # a reward object of the caller's own: compute_reward(m, s) only

    def _host_reward_value(self, traj, n):
        """sum over the pre-propagation states t < n of the host reward terms (pilco.py:133 accumulates the same way)."""
        E, tot = self.state_dim, 0.0
        for t in range(int(n)):
            m, s = traj[t, :E].reshape(1, E), traj[t, E:].reshape(E, E)
            for c, r in self._host_reward_terms():
                tot += c * float(np.ravel(r.compute_reward(m, s)[0])[0])
        return tot

    def trajectory_objective(self, traj):
        """What predict() adds to the device reward as a function of the state trajectory -- the host reward terms -- and
        its cotangent seeds d / d (m_t, s_t) for the native reverse sweep (pilco_rollout_grad_seeded).  None if a host term
        has no compute_reward_grad (optimize_policy then differentiates training_loss by finite differences)."""
        host = self._host_reward_terms()
        E, H = self.state_dim, traj.shape[0] - 1
        seeds, value = np.zeros_like(traj), 0.0
        for c, r in host:
            if not hasattr(r, "compute_reward_grad"):
                return None
            for t in range(H):
                v, dm, ds = r.compute_reward_grad(traj[t, :E].reshape(1, E), traj[t, E:].reshape(E, E))
                value += c * float(v)
                seeds[t, :E] += c * np.ravel(dm)
                seeds[t, E:] += c * np.ravel(ds)
        return value, seeds

    def _refuse_mlp(self, who):
        """a network policy has no action moments: the moment-matching methods refuse it before any device call"""
        if self.control_dim > 0 and isinstance(self.controller, controllers.MlpController):
            raise NotImplementedError("%s: moment matching needs the action's moments in closed form, which an MlpController "
                                      "does not have; use the particle paths (sample_trajectories, particle_value_and_gradient, "
                                      "optimize_policy(objective=\"particles\"))" % who)

    # pilco.py:47-50
    def training_loss(self):
        self._refuse_mlp("training_loss")
        return -self.predict(self.m_init, self.S_init, self.horizon)[2]

    # pilco.py:52-73 (the pandas pretty-printing is cosmetic and omitted)
    def optimize_models(self, maxiter=200, restarts=1, verbose=True):
        self.mgpr.optimize(restarts=restarts)
        if verbose:
            print('-----Learned models------')
            for i, model in enumerate(self.mgpr.models):
                print('GP%d lengthscales %s variance %.3g noise %.3g' % (
                    i, np.array2string(np.asarray(model.kernel.lengthscales.numpy()), precision=3),
                    float(model.kernel.variance.numpy()), float(model.likelihood.variance.numpy())))

    # pilco.py:75-113
    def optimize_policy(self, maxiter=50, restarts=1, verbose=True, objective="moment_matching", particle_options=None):
        """objective="particles" (extension): maximise the particle return of particle_value_and_gradient on fixed initial
        particles and draws instead of the moment-matched reward; particle_options: num_particles, seed, observation_noise.
        An MlpController is optimised with objective="particles" only: the default objective raises NotImplementedError."""
        from ..training import optimize_policy
        return optimize_policy(self, maxiter=maxiter, restarts=restarts, verbose=verbose, objective=objective,
                               particle_options=particle_options)

    # pilco.py:115-116
    def value_and_gradient(self, seed_fn=None):
        """(reward, grads) of the rollout reward w.r.t. the controller parameters: grads = (dW, db) for a LinearController,
        (dX, dY, dlengthscales) for an RbfController.  The reference obtains it from TensorFlow's reverse mode through the
        tf.while_loop (pilco/models/pilco.py:85-90,126-135); here the whole reverse sweep is native (pilco_rollout_grad /
        pilco_rollout_grad_rbf) and deterministic: the same inputs give bitwise the same gradient.
        seed_fn(traj (H+1, E+E*E)) -> cotangent seeds d objective / d (m_t, s_t) for an objective beyond the additive
        reward (the returned reward is the additive part; the gradients are those of additive reward + seeded objective)."""
        self._refuse_mlp("value_and_gradient")
        ctl = self.controller
        linear = isinstance(ctl, controllers.LinearController)
        if not linear and not isinstance(ctl, controllers.RbfController):
            raise TypeError("analytic policy gradient: LinearController or RbfController")
        self.mgpr._user_factors = None
        self.mgpr._ensure_factorized()
        if linear:
            r, dW, db = self.ctx.rollout_grad(self._policy_spec(), self._reward_terms(), self.m_init, self.S_init, self.horizon, seed_fn=seed_fn)
            return r, (dW.reshape(ctl.W.shape), db.reshape(ctl.b.shape))
        r, dX, dY, dl = self.ctx.rollout_grad_rbf(self._policy_spec(), self._reward_terms(), self.m_init, self.S_init, self.horizon,
                                                  ctl.X, ctl.Y, ctl.lengthscales, ctl.noise, seed_fn=seed_fn)
        return r, (dX, dY, dl)

    def _initial_particles(self, m_x, s_x, num_particles, seed):
        """x0 = m_x + z sqrt(s_x): z from np.random.default_rng(seed), the symmetric square root, eigenvalues clipped at zero"""
        E = self.state_dim
        m = np.asarray(m_x, np.float64).reshape(1, E)
        w, V = np.linalg.eigh(0.5 * (np.asarray(s_x, np.float64).reshape(E, E) + np.asarray(s_x, np.float64).reshape(E, E).T))
        root = (V * np.sqrt(np.clip(w, 0.0, None))) @ V.T
        return m + np.random.default_rng(seed).standard_normal((int(num_particles), E)) @ root

    def _check_particle_dynamics(self, who, dynamics, conditioned=False):
        """the dynamics argument of the particle methods, before any device call; conditioned: the method has the
        path-conditioned rollout (sample_trajectories; its gradient does not exist)"""
        if dynamics not in ("marginal", "function", "conditioned"):
            raise ValueError("%s: dynamics must be 'marginal', 'function' or 'conditioned', got %r" % (who, dynamics))
        if dynamics == "conditioned" and not conditioned:
            raise NotImplementedError("%s: dynamics='conditioned' has no gradient; the path-conditioned rollout is "
                                      "sample_trajectories' (docs/particle_conditioned.md)" % who)
        if dynamics == "function" and isinstance(self.mgpr, SMGPR):
            raise NotImplementedError("%s: dynamics='function' needs an exact GP (MGPR); function samples of a "
                                      "sparse model are not supported" % who)

    def particle_value_and_gradient(self, m_x=None, s_x=None, n=None, num_particles=1000, seed=0, eps=None, x0=None,
                                    observation_noise=False, return_dx0=False, dynamics="marginal", num_features=512,
                                    function_draws=None):
        """Extension: (reward, grads) of the PARTICLE return -- sample_trajectories(...).reward_steps.sum() on the same initial
        particles and draws -- w.r.t. the controller parameters, on the device (pilco_rollout_particles_grad / _grad_rbf;
        docs/particle_gradients.md).  grads has the structure value_and_gradient returns: (dW, db) for a LinearController,
        (dX, dY, dlengthscales) for an RbfController, (dW1, db1, dW2, db2) in the parameters' shapes for an MlpController
        (pilco_rollout_particles_grad_mlp / _fn_grad_mlp; docs/particle_mlp.md), () without a controller.  m_x, s_x, n default to m_init, S_init and
        horizon; x0, eps, seed and observation_noise are those of sample_trajectories.  With x0 (or seed) and the draws fixed
        the value is a deterministic, smooth function of the parameters (common random numbers).  return_dx0: a third
        result (P, E), row p the gradient of particle p's own return w.r.t. its initial state.  Any reward term evaluated on
        the host raises NotImplementedError, event terms included: an indicator has no gradient.
        dynamics="function": the return of sample_trajectories(dynamics="function") on num_features features or the caller's
        function_draws (pilco_rollout_particles_fn_grad / _grad_rbf; docs/particle_fn_gradients.md); eps is then read only
        with observation_noise.  Exact GP only: an SMGPR raises NotImplementedError.  Any other value raises ValueError."""
        self._check_particle_dynamics("particle_value_and_gradient", dynamics)
        if self._host_reward_terms():
            raise NotImplementedError("particle_value_and_gradient: reward terms evaluated on the host (events included) are not "
                                      "part of the differentiated objective")
        ctl = self.controller if self.control_dim > 0 else None
        linear = isinstance(ctl, controllers.LinearController)
        mlp = isinstance(ctl, controllers.MlpController)
        if ctl is not None and not linear and not mlp and not isinstance(ctl, controllers.RbfController):
            raise TypeError("particle policy gradient: LinearController, RbfController or MlpController")
        m_x = self.m_init if m_x is None else m_x
        s_x = self.S_init if s_x is None else s_x
        n = self.horizon if n is None else int(n)
        if x0 is None:
            x0 = self._initial_particles(m_x, s_x, num_particles, seed)
        x0 = np.asarray(x0, np.float64).reshape(-1, self.state_dim)
        self.mgpr._user_factors = None
        self.mgpr._ensure_factorized()
        kw = dict(eps=eps, seed=seed, observation_noise=observation_noise, want_dx0=return_dx0)
        if dynamics == "function":
            if function_draws is not None:
                function_draws = {k: function_draws[k] for k in ("omega", "phase", "w", "xi")}
            kw.update(num_features=num_features, function_draws=function_draws)
            if mlp:
                r, _, *g, dx0, _ = self.ctx.rollout_particles_fn_grad_mlp(self._policy_spec(), self._reward_terms(), x0, n, **kw)
                grads = tuple(a.reshape(p.shape) for a, p in zip(g, (ctl.W1, ctl.b1, ctl.W2, ctl.b2)))
            elif ctl is None or linear:
                r, _, dW, db, dx0, _ = self.ctx.rollout_particles_fn_grad(self._policy_spec(), self._reward_terms(), x0, n, **kw)
                grads = (dW.reshape(ctl.W.shape), db.reshape(ctl.b.shape)) if linear else ()
            else:
                r, _, dX, dY, dl, dx0, _ = self.ctx.rollout_particles_fn_grad_rbf(self._policy_spec(), self._reward_terms(), x0, n,
                                                                                  ctl.X, ctl.Y, ctl.lengthscales, ctl.noise, **kw)
                grads = (dX, dY, dl)
        elif mlp:
            r, _, *g, dx0 = self.ctx.rollout_particles_grad_mlp(self._policy_spec(), self._reward_terms(), x0, n, **kw)
            grads = tuple(a.reshape(p.shape) for a, p in zip(g, (ctl.W1, ctl.b1, ctl.W2, ctl.b2)))
        elif ctl is None or linear:
            r, _, dW, db, dx0 = self.ctx.rollout_particles_grad(self._policy_spec(), self._reward_terms(), x0, n, **kw)
            grads = (dW.reshape(ctl.W.shape), db.reshape(ctl.b.shape)) if linear else ()
        else:
            r, _, dX, dY, dl, dx0 = self.ctx.rollout_particles_grad_rbf(self._policy_spec(), self._reward_terms(), x0, n,
                                                                        ctl.X, ctl.Y, ctl.lengthscales, ctl.noise, **kw)
            grads = (dX, dY, dl)
        return (r, grads, dx0) if return_dx0 else (r, grads)

    def compute_action(self, x_m):
        return self.controller.compute_action(x_m, np.zeros([self.state_dim, self.state_dim]))[0]

    def linearize(self, x, u=None):
        """Extension: the learned dynamics linearised at the state(s) x (E,) or (Nt, E) and the action(s) u (U,) or (Nt, U)
        -- by default the controller's compute_action(x); a model without control inputs takes no u.  One device call for
        the model (MGPR.predict_f_jacobian at [x, u]); the default action and K cost one compute_action call and one host
        action_jacobian (for an RbfController a solve for beta) per state.  Returns a Linearization.  ValueError for a u
        given to a model without control, a u of another shape than (Nt, control_dim), or no u and no controller."""
        E, Ud = self.state_dim, self.control_dim
        x = np.asarray(x, np.float64)
        single = x.ndim == 1
        if x.ndim > 2 or x.shape[-1] != E:
            raise ValueError(f"linearize: x must be ({E},) or (Nt, {E})")
        X = x.reshape(-1, E)
        Nt = X.shape[0]
        K = None
        if Ud == 0:
            if u is not None:
                raise ValueError("linearize: the model has no control input, u must be None")
            U = np.empty((Nt, 0))
        elif u is None:
            if self.controller is None:
                raise ValueError("linearize: no controller, give u")
            U = np.stack([np.asarray(self.compute_action(X[t:t + 1]), np.float64).reshape(-1) for t in range(Nt)])
            K = np.stack([self.controller.action_jacobian(X[t]) for t in range(Nt)])
        else:
            U = np.asarray(u, np.float64)
            if U.shape != ((Ud,) if single else (Nt, Ud)):
                raise ValueError(f"linearize: u must be {(Ud,) if single else (Nt, Ud)}, got {U.shape}")
            U = U.reshape(Nt, Ud)
        mean, var, dmean, dvar = (np.asarray(a) for a in self.mgpr.predict_f_jacobian(np.hstack([X, U])))
        A = np.eye(E)[None] + dmean[..., :E]          # the GP predicts differences (pilco.py:138-153)
        B = dmean[..., E:]
        out = dict(x_next=X + mean, var=var, A=A, B=B, dvar_dx=dvar[..., :E], dvar_du=dvar[..., E:], u=U, K=K,
                   A_cl=None if K is None else A + B @ K)
        if single:
            out = {k: (None if v is None else v[0]) for k, v in out.items()}
        return Linearization(**out)

    # pilco.py:118-136
    def predict(self, m_x, s_x, n):
        self._refuse_mlp("predict")
        self.mgpr._user_factors = None
        self.mgpr._ensure_factorized()
        if not self._host_reward_terms():
            return self.ctx.rollout(self._policy_spec(), self._reward_terms(), m_x, s_x, int(n))
        M, S, R, _ = self.predict_trajectory(m_x, s_x, n)
        return M, S, R

    def predict_trajectory(self, m_x, s_x, n):
        """Extension: also returns the (n+1, E + E*E) per-step states."""
        self._refuse_mlp("predict_trajectory")
        self.mgpr._user_factors = None
        self.mgpr._ensure_factorized()
        M, S, R, traj = self.ctx.rollout(self._policy_spec(), self._reward_terms(), m_x, s_x, int(n), want_traj=True)
        if self._host_reward_terms():
            R = R + self._host_reward_value(traj, n)
        return M, S, R, traj

    def sample_trajectories(self, m_x, s_x, n, num_particles=1000, seed=0, eps=None, x0=None, observation_noise=False,
                            return_particles=False, events=None, dynamics="marginal", num_features=512, function_draws=None,
                            jitter=1e-8, eps_obs=None):
        """Extension: num_particles trajectories of n steps sampled through the learned dynamics on the device
        (pilco_rollout_particles), to hold against the Gaussians predict() propagates.  Every particle acts with
        compute_action(x) and moves by a draw from the GP posterior at [x, u] (latent variance; observation_noise adds the
        likelihood variance).  x0 (P, E): the initial particles; otherwise x0 = m_x + z sqrt(s_x) with z from
        np.random.default_rng(seed) and the symmetric square root of s_x (eigenvalues clipped at zero: s_x = 0 works).
        eps (n, P, E): the standard-normal draws of the steps; otherwise generated on the device from ``seed``.  An SMGPR
        runs on the shared inducing inputs of the rollout.  events: a list of K events counted on the device
        (pilco_rollout_particles_events) -- objects with event_spec() (pilco_amd.safe's constraints) or dicts
        dict(clauses=[(dim, low, high), ...], complement=bool) -- which fill event_counts, event_prob and first_hit of the
        result.  A host reward term that offers event_spec() adds c * counts[t] / P to reward_steps[t], the mean over the
        particles of c * 1[hit]: the term at zero covariance.  Such terms are counted with the caller's events, at most 8
        together.  Any other host reward term raises NotImplementedError.  Returns a ParticleTrajectories.
        dynamics="marginal": every step is an independent draw from the posterior marginal at [x, u] (above).
        dynamics="function": every particle draws ONE dynamics function from the GP posterior -- num_features random Fourier
        features conditioned on the data pathwise, or the caller's function_draws (the result's function_draws fed back
        reproduces every output bitwise) -- and follows it deterministically (pilco_rollout_particles_fn,
        docs/particle_functions.md); eps is then used only with observation_noise (the result's eps is None without it).
        Exact GP only: an SMGPR raises NotImplementedError.
        dynamics="conditioned": every step is drawn conditioned on the particle's own earlier visited points -- the exact
        joint posterior along the trajectory, for MGPR and SMGPR alike (pilco_rollout_particles_cond,
        docs/particle_conditioned.md).  eps is the step stream of "marginal" (the same seed gives the same first step up to
        the jitter); observation noise is a second stream, eps_obs (n, P, E) or generated, which never enters the
        conditioning.  jitter (relative to the kernel variance) is added to the path covariance before it is factored.  With
        return_particles the result carries eps_obs, path_cov and path_factor.  n is at most 128.  num_features (other than
        its default) and function_draws raise ValueError here.  Any other value of dynamics raises ValueError."""
        self._check_particle_dynamics("sample_trajectories", dynamics, conditioned=True)
        if dynamics == "conditioned" and (num_features != 512 or function_draws is not None):
            raise ValueError("sample_trajectories: num_features and function_draws belong to dynamics='function', not 'conditioned'")
        if dynamics != "conditioned" and eps_obs is not None:
            raise ValueError("sample_trajectories: eps_obs belongs to dynamics='conditioned'")
        host = self._host_reward_terms()
        if any(not hasattr(r, "event_spec") for _, r in host):
            raise NotImplementedError("sample_trajectories: reward terms evaluated on the host are not supported on particles; "
                                      "ask for return_particles=True and evaluate them on the returned particles")
        K = 0 if events is None else len(events)
        table = (list(events) if events is not None else []) + [r for _, r in host]
        E = self.state_dim
        if x0 is None:
            x0 = self._initial_particles(m_x, s_x, num_particles, seed)
        x0 = np.asarray(x0, np.float64).reshape(-1, E)
        self.mgpr._user_factors = None
        self.mgpr._ensure_factorized()
        if dynamics == "function":
            return self._sample_function_trajectories(x0, int(n), eps, seed, observation_noise, return_particles, events, K, table,
                                                      host, num_features, function_draws)
        if dynamics == "conditioned":
            mean, cov, rew, parts, used, counts, first, zeta, pcov, pfac = self.ctx.rollout_particles_cond(
                self._policy_spec(), self._reward_terms(), x0, int(n), eps=eps, seed=seed, observation_noise=observation_noise,
                want_particles=return_particles, events=table if (events is not None or host) else None, jitter=jitter,
                eps_obs=eps_obs, want_path=return_particles)
            if host:   # the mean over the particles of c * 1[hit] at the pre-step states
                for j, (c, _) in enumerate(host):
                    for t in range(int(n)):
                        rew[t] += c * float(counts[t, K + j]) / x0.shape[0]
            kw = dict(eps_obs=zeta if return_particles else None, path_cov=pcov, path_factor=pfac)
            if events is None:
                return ParticleTrajectories(mean, cov, rew, parts, used, **kw)
            return ParticleTrajectories(mean, cov, rew, parts, used, np.ascontiguousarray(counts[:, :K]),
                                        np.ascontiguousarray(first[:, :K]), **kw)
        out = self.ctx.rollout_particles(self._policy_spec(), self._reward_terms(), x0, int(n), eps=eps, seed=seed,
                                         observation_noise=observation_noise, want_particles=return_particles,
                                         events=table if (events is not None or host) else None)
        mean, cov, rew, parts, used = out[:5]
        if host:   # the mean over the particles of c * 1[hit] at the pre-step states
            counts, P = out[5], x0.shape[0]
            for j, (c, _) in enumerate(host):
                for t in range(int(n)):
                    rew[t] += c * float(counts[t, K + j]) / P
        if events is None:
            return ParticleTrajectories(mean, cov, rew, parts, used)
        return ParticleTrajectories(mean, cov, rew, parts, used, np.ascontiguousarray(out[5][:, :K]), np.ascontiguousarray(out[6][:, :K]))

    def _sample_function_trajectories(self, x0, n, eps, seed, observation_noise, return_particles, events, K, table, host,
                                      num_features, function_draws):
        """sample_trajectories(dynamics="function") behind its checks: x0 (P, E) and the event table are ready."""
        if function_draws is not None:
            function_draws = {k: function_draws[k] for k in ("omega", "phase", "w", "xi")}
        mean, cov, rew, parts, used, counts, first, draws = self.ctx.rollout_particles_fn(
            self._policy_spec(), self._reward_terms(), x0, n, num_features=num_features, function_draws=function_draws, eps=eps,
            seed=seed, observation_noise=observation_noise, want_particles=return_particles,
            events=table if (events is not None or host) else None, want_draws=return_particles)
        if host:   # the mean over the particles of c * 1[hit] at the pre-step states
            P = x0.shape[0]
            for j, (c, _) in enumerate(host):
                for t in range(n):
                    rew[t] += c * float(counts[t, K + j]) / P
        if events is None:
            return ParticleTrajectories(mean, cov, rew, parts, used, function_draws=draws)
        return ParticleTrajectories(mean, cov, rew, parts, used, np.ascontiguousarray(counts[:, :K]),
                                    np.ascontiguousarray(first[:, :K]), function_draws=draws)

    # pilco.py:138-153
    def propagate(self, m_x, s_x):
        self._refuse_mlp("propagate")
        self.mgpr._user_factors = None
        self.mgpr._ensure_factorized()
        return self.ctx.propagate(self._policy_spec(), m_x, s_x)

    # pilco.py:155-156
    def compute_reward(self):
        self._refuse_mlp("compute_reward")
        return -self.training_loss()

    @property
    def maximum_log_likelihood_objective(self):
        return -self.training_loss()

    @property
    def trainable_parameters(self):
        ps = list(self.mgpr.trainable_parameters)
        if self.controller is not None:
            own = getattr(type(self.controller), "trainable_parameters", None)    # an RbfController lists centres, targets, lengthscales
            ps += list(self.controller.trainable_parameters) if own is not None else [p for p in parameters_of(self.controller) if p.trainable]
        return ps
