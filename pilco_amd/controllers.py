"""Controllers with the reference's interface (/root/reference/pilco/controllers.py):
``compute_action(m, s, squash=True) -> (M (1,k), S (k,k), V (d,k))`` and
``randomize()``.  Arithmetic runs on the device (k_glue in csrc/glue.hip)."""
from __future__ import annotations

import numpy as np

from . import _lib
from .params import Parameter


def squash_sin(m, s, max_action=None, ctx=None):
    """Moments of e*sin(x), x ~ N(m, s)  (controllers.py:13-36).

    Evaluated on the device as an identity linear map followed by the squashing
    stage of the controller kernel."""
    m = np.asarray(m, np.float64).reshape(1, -1)
    k = m.shape[1]
    ctx = ctx or _lib.get_context()
    spec = dict(kind=_lib.POLICY_LINEAR, state_dim=k, control_dim=k, W=np.eye(k), b=np.zeros(k),
                max_action=np.ones(k) if max_action is None else max_action, squash=True)
    return ctx.policy_action(spec, m, s)


class LinearController:
    """controllers.py:39-63."""

    def __init__(self, state_dim, control_dim, max_action=1.0, ctx=None):
        self.state_dim = state_dim
        self.control_dim = control_dim
        self.W = Parameter(np.random.rand(control_dim, state_dim), name="W")
        self.b = Parameter(np.random.rand(1, control_dim), name="b")
        self.max_action = max_action
        self._ctx = ctx

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.resolve_ctx(self)
        return self._ctx

    def policy_spec(self, squash=True):
        return dict(kind=_lib.POLICY_LINEAR, state_dim=self.state_dim, control_dim=self.control_dim,
                    W=self.W.numpy(), b=self.b.numpy().reshape(-1), max_action=self.max_action, squash=squash)

    def compute_action(self, m, s, squash=True):
        return self.ctx.policy_action(self.policy_spec(squash), m, s)

    def action_jacobian(self, x):
        """d u / d x (U, E) of the deterministic action u = compute_action(x, 0)[0] = max_action * sin(x W^T + b) at the
        state x (E,) (extension; host NumPy, docs/particles.md states the action)."""
        x = np.asarray(x, np.float64).reshape(-1)
        W = np.asarray(self.W.numpy(), np.float64)
        a = W @ x + np.asarray(self.b.numpy(), np.float64).reshape(-1)
        scale = np.broadcast_to(np.asarray(self.max_action, np.float64).reshape(-1), a.shape)
        return (scale * np.cos(a))[:, None] * W

    def randomize(self):
        mean, sigma = 0, 1
        self.W.assign(mean + sigma * np.random.normal(size=self.W.shape))
        self.b.assign(mean + sigma * np.random.normal(size=self.b.shape))

    @property
    def trainable_parameters(self):
        return [p for p in (self.W, self.b) if p.trainable]


class _PolicyData(Parameter):
    """The centres X / targets Y of an RbfController as gpflow-like Parameters (controllers.py:70-73: both are
    trainable ``Parameter``s of the reference's FakeGPR); values live in the policy GP, ``assign`` goes through set_data."""

    def __init__(self, gp, which, name):
        self._gp = None                      # (the base constructor's `self._v = ...` must not re-seat the GP's data)
        self._which = which
        Parameter.__init__(self, gp._X if which == 0 else gp._Y, name=name)
        self._gp = gp

    @property
    def _v(self):
        return self._gp._X if self._which == 0 else self._gp._Y

    @_v.setter
    def _v(self, value):
        if getattr(self, "_gp", None) is None:
            return
        value = np.array(value, dtype=np.float64)
        self._gp.set_data((value, self._gp._Y) if self._which == 0 else (self._gp._X, value))


class RbfController:
    """RBF network controller = deterministic GP (controllers.py:80-129; Deisenroth et al. 2015, sec. 5.3.2).

    In the reference this is an MGPR subclass whose ``compute_action`` calls
    ``predict_given_factorizations(m, s, 0.0 * iK, beta)`` and subtracts ``diag(variance - 1e-6)``.
    Here the policy GP lives in device slot 1 (PILCO_SLOT_POLICY) and is evaluated by the same
    moment-matching kernels with the iK stream switched off."""

    def __init__(self, state_dim, control_dim, num_basis_functions, max_action=1.0, ctx=None):
        from .models.mgpr import MGPR

        class _PolicyGP(MGPR):
            _slot = _lib.SLOT_POLICY

        self.state_dim = state_dim
        self.control_dim = control_dim
        self.num_basis_functions = num_basis_functions
        self.max_action = max_action
        data = (np.random.randn(num_basis_functions, state_dim), 0.1 * np.random.randn(num_basis_functions, control_dim))
        self._gp = _PolicyGP(data, ctx=ctx)
        self.create_models(data)
        self.centres = _PolicyData(self._gp, 0, "DataX")     # shared by every output (controllers.py:104-106)
        self.targets = _PolicyData(self._gp, 1, "DataY")

    # -- controllers.py:96-106
    def create_models(self, data):
        """One model per control dimension over shared centres: unit kernel variance (fixed), likelihood variance 1e-4
        (fixed), lengthscales one with the lower bound 1e-3 of the reference's transform."""
        if data is not None and (np.shape(data[0]) != np.shape(self._gp._X) or np.shape(data[1]) != np.shape(self._gp._Y)
                                 or not (np.array_equal(data[0], self._gp._X) and np.array_equal(data[1], self._gp._Y))):
            self._gp.set_data(data)                          # the reference builds the models FROM this data (controllers.py:96-106)
            self.num_basis_functions = self._gp.num_datapoints
        self._gp.create_models(data)
        for model in self._gp.models:
            model.kernel.variance.assign(1.0)               # controllers.py:92-93
            model.kernel.variance.trainable = False
            model.likelihood.variance.assign(1e-4)          # FakeGPR, controllers.py:67,76-77
            model.likelihood.variance.trainable = False
            model.kernel.lengthscales.lower = 1e-3          # positive(lower=1e-3), controllers.py:100
        self._gp._invalidate()

    def __getattr__(self, name):
        """The reference's RbfController IS an MGPR (controllers.py:80): whatever of that surface is not spelled out below
        (num_outputs, predict_given_factorizations, centralized_input, K, data, ...) is the policy GP's."""
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._gp, name)

    # -- the MGPR surface the reference's callers use on an RbfController
    @property
    def models(self):
        return self._gp.models

    @property
    def ctx(self):
        return self._gp.ctx

    def set_data(self, data):
        self._gp.set_data(data)
        self.num_basis_functions = self._gp.num_datapoints

    @property
    def X(self):
        return self._gp.X

    @property
    def Y(self):
        return self._gp.Y

    @property
    def lengthscales(self):
        return self._gp.lengthscales

    @property
    def variance(self):
        return self._gp.variance

    @property
    def noise(self):
        return self._gp.noise

    def calculate_factorizations(self):
        return self._gp.calculate_factorizations()

    def sync(self):
        """Push centres / targets / lengthscales to the device and refresh beta."""
        self._gp._user_factors = None
        self._gp._ensure_factorized()

    def policy_spec(self, squash=True):
        self.sync()
        return dict(kind=_lib.POLICY_RBF, state_dim=self.state_dim, control_dim=self.control_dim,
                    max_action=self.max_action, squash=squash)

    def compute_action(self, m, s, squash=True):
        return self.ctx.policy_action(self.policy_spec(squash), m, s)

    def action_jacobian(self, x):
        """d u / d x (U, E) of the deterministic action u = compute_action(x, 0)[0] at the state x (E,) (extension; host
        NumPy): u_k = max_action_k exp(-5e-7) sin(a_k), a_k = sum_i beta_ki k_k(x, c_i) with unit signal variance and
        beta_k = (K_k + noise_k I)^-1 y_k (docs/particles.md; exp(-5e-7) is the 1e-6 variance the reference leaves at s = 0)."""
        x = np.asarray(x, np.float64).reshape(-1)
        C, Y = np.asarray(self._gp._X, np.float64), np.asarray(self._gp._Y, np.float64)
        ls, noise = np.asarray(self._gp.lengthscales, np.float64), np.asarray(self._gp.noise, np.float64).reshape(-1)
        U = Y.shape[1]
        scale = np.broadcast_to(np.asarray(self.max_action, np.float64).reshape(-1), (U,)) * np.exp(-5e-7)
        J = np.empty((U, x.size))
        for k in range(U):
            d = (C[:, None, :] - C[None, :, :]) / ls[k]
            K = np.exp(-0.5 * np.sum(d * d, axis=-1)) + noise[k] * np.eye(C.shape[0])
            beta = np.linalg.solve(K, Y[:, k])
            diff = (C - x) / ls[k] ** 2                                   # (bf, E): d k_i / d x = k_i (c_i - x) / l^2
            g = beta * np.exp(-0.5 * np.sum(((C - x) / ls[k]) ** 2, axis=-1))
            J[k] = scale[k] * np.cos(g.sum()) * (g @ diff)
        return J

    def randomize(self):
        """controllers.py:123-129, with its draw order from NumPy's global generator: model by model the centres (the
        shared X Parameter is re-assigned by every model, so the last model's draw stays), that model's targets, that
        model's lengthscales -- a seeded restart starts where the reference's starts for any control_dim."""
        bf, U = self._gp.X.shape[0], self._gp.Y.shape[1]
        Y = np.empty((bf, U))
        scale = np.broadcast_to(np.asarray(self.max_action, np.float64).reshape(-1), (U,)) if np.size(self.max_action) in (1, U) else None
        for k, m in enumerate(self.models):
            X = np.random.normal(size=self._gp.X.shape)
            draw = np.random.normal(size=(bf, 1))
            Y[:, k:k + 1] = (self.max_action if scale is None else scale[k]) / 10 * draw
            m.kernel.lengthscales.assign(1 + 0.1 * np.random.normal(size=m.kernel.lengthscales.shape))
        self._gp.set_data((X, Y))

    @property
    def trainable_parameters(self):
        """Centres, targets and per-output lengthscales -- the reference's trainable set (controllers.py:70-73,100)."""
        return [p for p in [self.centres, self.targets] + [m.kernel.lengthscales for m in self.models] if p.trainable]


class MlpController:
    """Extension (docs/particle_mlp.md): a neural-network policy for the PARTICLE paths -- one hidden layer of tanh units,

        h = tanh(W1 x + b1),   s = W2 h + b2,   u = max_action * sin(s)  (squash)  or  s.

    A network has no closed-form action moments: sample_trajectories, particle_value_and_gradient and
    optimize_policy(objective="particles") work with it, the moment-matching methods raise NotImplementedError.  The
    parameters travel to the device with every particle call (Context.set_policy_mlp keeps the host copy)."""

    def __init__(self, state_dim, control_dim, num_hidden=32, max_action=1.0, ctx=None):
        if not 1 <= int(num_hidden) <= _lib.MAX_MLP_HIDDEN:
            raise ValueError("MlpController: num_hidden must be 1..%d" % _lib.MAX_MLP_HIDDEN)
        self.state_dim = state_dim
        self.control_dim = control_dim
        self.num_hidden = int(num_hidden)
        self.W1 = Parameter(np.zeros((self.num_hidden, state_dim)), name="W1")
        self.b1 = Parameter(np.zeros((self.num_hidden,)), name="b1")
        self.W2 = Parameter(np.zeros((control_dim, self.num_hidden)), name="W2")
        self.b2 = Parameter(np.zeros((1, control_dim)), name="b2")
        self.max_action = max_action
        self._ctx = ctx
        self.randomize()

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.resolve_ctx(self)
        return self._ctx

    def _host(self):
        return (np.asarray(self.W1.numpy(), np.float64), np.asarray(self.b1.numpy(), np.float64).reshape(-1),
                np.asarray(self.W2.numpy(), np.float64), np.asarray(self.b2.numpy(), np.float64).reshape(-1))

    def _scale(self):
        return np.broadcast_to(np.asarray(self.max_action, np.float64).reshape(-1), (self.control_dim,))

    def policy_spec(self, squash=True):
        par = self._host()
        ctx = self.ctx
        sent = ctx.policy_mlp_set   # a context holds ONE network: another controller may have set its own since
        if sent is None or any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(par, sent)):
            ctx.set_policy_mlp(*par)
        return dict(kind=_lib.POLICY_MLP, state_dim=self.state_dim, control_dim=self.control_dim, max_action=self.max_action,
                    squash=squash)

    def compute_action(self, m, s, squash=True):
        """The deterministic action at m (1, E), on the host: (M (1, U), zeros (U, U), zeros (E, U)).  Any non-zero s raises
        NotImplementedError: the moments of a network's action under a Gaussian state have no closed form."""
        if np.any(np.asarray(s, np.float64) != 0.0):
            raise NotImplementedError("MlpController.compute_action: no action moments under a state covariance; an MlpController "
                                      "serves the particle paths (optimize_policy(objective=\"particles\"), sample_trajectories)")
        W1, b1, W2, b2 = self._host()
        x = np.asarray(m, np.float64).reshape(-1)
        a = W2 @ np.tanh(W1 @ x + b1) + b2
        M = self._scale() * np.sin(a) if squash else a
        return M.reshape(1, -1), np.zeros((self.control_dim, self.control_dim)), np.zeros((self.state_dim, self.control_dim))

    def action_jacobian(self, x):
        """d u / d x (U, E) of the deterministic action u = compute_action(x, 0)[0] at the state x (E,) (host NumPy)."""
        W1, b1, W2, b2 = self._host()
        x = np.asarray(x, np.float64).reshape(-1)
        h = np.tanh(W1 @ x + b1)
        a = W2 @ h + b2
        return (self._scale() * np.cos(a))[:, None] * ((W2 * (1.0 - h * h)) @ W1)

    def randomize(self):
        """W1 ~ N(0, 1 / E), W2 ~ N(0, 1 / num_hidden), b1 = 0, b2 ~ N(0, 1), from NumPy's global generator in this order."""
        self.W1.assign(np.random.normal(size=self.W1.shape) / np.sqrt(self.state_dim))
        self.W2.assign(np.random.normal(size=self.W2.shape) / np.sqrt(self.num_hidden))
        self.b1.assign(np.zeros(self.b1.shape))
        self.b2.assign(np.random.normal(size=self.b2.shape))

    @property
    def trainable_parameters(self):
        return [p for p in (self.W1, self.b1, self.W2, self.b2) if p.trainable]
