"""MGPR: E independent squared-exponential GPs sharing their inputs, with the
analytic moment-matching prediction at Gaussian inputs.

Same public surface as the reference's ``pilco.models.MGPR``
(/root/reference/pilco/models/mgpr.py:17-190); the arithmetic runs in
libpilco_hip.so on the MI355X.  Differences from the reference, all API-legal:
the factorisation is cached on the device and recomputed only when data or
hyper-parameters change (the reference recomputes it on every
``predict_on_noisy_inputs`` call, mgpr.py:77-79).
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..params import GPModelView, parameters_of, tensor_value


def randomize(model, mean=1, sigma=0.01):
    """mgpr.py:8-15: a fresh start for one output's model -- Normal(mean, sigma) draws from NumPy's global generator for the
    lengthscales, the kernel variance and (only if trainable) the likelihood variance, in that order."""
    k, lik = model.kernel, model.likelihood.variance
    k.lengthscales.assign(mean + sigma * np.random.normal(size=np.shape(k.lengthscales.numpy())))
    k.variance.assign(mean + sigma * np.random.normal(size=np.shape(k.variance.numpy())))
    if lik.trainable:
        lik.assign(mean + sigma * np.random.normal())


class MGPR:
    _slot = _lib.SLOT_DYNAMICS

    def __init__(self, data, name=None, ctx=None):
        self.name = name
        self._ctx = ctx
        X, Y = np.asarray(data[0], np.float64), np.asarray(data[1], np.float64)
        self.num_outputs = Y.shape[1]
        self.num_dims = X.shape[1]
        self.num_datapoints = X.shape[0]
        self._X, self._Y = X.copy(), Y.copy()
        self._data_dirty = True
        self._hyp_dirty = True
        self._user_factors = None
        self.create_models(data)
        self.optimizers = []

    # -- reference: mgpr.py:28-36
    def create_models(self, data):
        self.models = [GPModelView(self, i, self.num_dims) for i in range(self.num_outputs)]

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.resolve_ctx(self)
        return self._ctx

    def _invalidate(self):
        self._hyp_dirty = True

    # -- reference: mgpr.py:38-45
    def set_data(self, data):
        X, Y = np.asarray(data[0], np.float64), np.asarray(data[1], np.float64)
        if X.shape[1] != self.num_dims or Y.shape[1] != self.num_outputs:
            raise ValueError("set_data: D and E are fixed at construction")
        self._X, self._Y = X.copy(), Y.copy()
        self.num_datapoints = X.shape[0]
        self._data_dirty = True

    # -- device synchronisation
    def _points(self):
        return self._X

    def _claim_slot(self):
        """The device slot is shared by every model of this kind on the context.  If another instance used it since
        this one last synchronised, everything this instance believes to be on the device is stale: push it all again
        (data, hyper-parameters, inducing inputs, factorisation)."""
        owner = self.ctx._slot_owner.get(self._slot)
        if owner is not self:
            self.ctx._slot_owner[self._slot] = self
            self._data_dirty = True
            self._hyp_dirty = True
            self._user_factors = None
            self._on_slot_taken()

    def _on_slot_taken(self):
        self._reset_inducing = True        # an SMGPR may have left inducing inputs in the slot

    def _sync(self):
        self._claim_slot()
        if self._data_dirty:
            self.ctx.gp_set_data(self._slot, self._X, self._Y, owner=self)
            self._data_dirty = False
            self._hyp_dirty = True
            if getattr(self, "_reset_inducing", False):
                self.ctx.gp_set_inducing(self._slot, None, owner=self)      # back to the exact GP (pilco_gp_set_data keeps M otherwise)
                self._reset_inducing = False
            self._after_set_data()
        if self._hyp_dirty:
            self.ctx.gp_set_hyp(self._slot, self.lengthscales, self.variance, self.noise, owner=self)
            self._hyp_dirty = False
            self._user_factors = None

    def _after_set_data(self):
        pass

    def _ensure_factorized(self):
        self._sync()
        if self._user_factors is None:
            self.ctx.gp_factorize(self._slot)                   # cached on the device: a no-op while nothing changed

    # -- reference: mgpr.py:47-75
    def optimize(self, restarts=1, keep="last"):
        """keep='last': the reference's end state (the last restart's fit stays, mgpr.py:59-75); keep='best': per output the
        better fit (extension).  See training.optimize_mgpr."""
        from ..training import optimize_mgpr
        return optimize_mgpr(self, restarts=restarts, keep=keep)

    # -- reference: mgpr.py:77-79
    def predict_on_noisy_inputs(self, m, s):
        self._user_factors = None
        self._ensure_factorized()
        return self.ctx.gp_predict(self._slot, m, s, self.num_dims, self.num_outputs)

    # -- gpflow GPR.predict_f / predict_y of the output models (mgpr.py:28-36 builds them), all outputs in one device call
    def _own_inducing(self):
        return None

    def _predict_points(self, Xnew, output=-1):
        """(mean, var) of the latent functions at Xnew (Nt, D): (Nt, E) each, or (Nt, 1) for one output."""
        self._user_factors = None
        self._ensure_factorized()
        mean, var = self.ctx.gp_predict_points(self._slot, np.asarray(Xnew, np.float64).reshape(-1, self.num_dims), self.num_dims,
                                               self.num_outputs, output, self._own_inducing())
        return tensor_value(mean.T), tensor_value(var.T)

    def _predict_points_cov(self, Xnew, output=-1):
        """(mean (Nt, E), cov (E, Nt, Nt)) of the latent functions at Xnew (Nt, D); E = 1 for one output."""
        self._user_factors = None
        self._ensure_factorized()
        mean, cov = self.ctx.gp_predict_points_cov(self._slot, np.asarray(Xnew, np.float64).reshape(-1, self.num_dims), self.num_dims,
                                                   self.num_outputs, output, self._own_inducing())
        return tensor_value(mean.T), tensor_value(cov)

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        """Every output's GPR.predict_f at Xnew (Nt, D): mean and latent variance, (Nt, E) each (extension); full_cov=True:
        the mean (Nt, E) and every output's posterior covariance between the test points, (E, Nt, Nt), GPflow's shapes
        (pilco_gp_predict_points_cov, docs/predict_cov.md)."""
        if full_output_cov:
            raise NotImplementedError("predict_f: full_output_cov=True is not supported (the outputs are independent)")
        if full_cov:
            return self._predict_points_cov(Xnew)
        return self._predict_points(Xnew)

    def _predict_f_samples(self, Xnew, output, num_samples, full_cov, full_output_cov, seed, draws, jitter, return_parts):
        if full_output_cov:
            raise NotImplementedError("predict_f_samples: full_output_cov=True is not supported (the outputs are independent)")
        X = np.asarray(Xnew, np.float64).reshape(-1, self.num_dims)
        S, Nt, rows = (1 if num_samples is None else int(num_samples)), X.shape[0], (self.num_outputs if output < 0 else 1)
        if draws is not None:
            draws = np.asarray(draws, np.float64)
            if num_samples is None and draws.shape == (Nt, rows):
                draws = draws[None]
            if draws.shape != (S, Nt, rows):
                raise ValueError("draws must be (num_samples, Nt, E) = (%d, %d, %d), got %s" % (S, Nt, rows, draws.shape))
        if full_cov:
            self._user_factors = None
            self._ensure_factorized()
            samples, parts = self.ctx.gp_sample_points(self._slot, X, self.num_dims, self.num_outputs, S, output, self._own_inducing(),
                                                       seed=seed, draws=draws, jitter=jitter, parts=True)
            parts = dict(mean=parts["mean"].T, cov=parts["cov"], chol=parts["chol"], draws=parts["draws"])
        else:   # the marginals: mean + sqrt(var) z on predict_f's bits, the same stream of normals
            from .._lib import philox_cov_normals
            mean, var = (np.asarray(v) for v in self._predict_points(X, output))
            if draws is None:
                draws = philox_cov_normals(seed, S, Nt, range(self.num_outputs) if output < 0 else [output])
            samples = mean[None] + np.sqrt(var)[None] * draws
            parts = dict(mean=mean, var=var, cov=None, chol=None, draws=draws)
        if num_samples is None:
            samples, parts["draws"] = samples[0], parts["draws"][0]
        if return_parts:
            return tensor_value(samples), {k: (v if v is None else tensor_value(v)) for k, v in parts.items()}
        return tensor_value(samples)

    def predict_f_samples(self, Xnew, num_samples=None, full_cov=True, full_output_cov=False, seed=0, draws=None, jitter=1e-6,
                          return_parts=False):
        """gpflow predict_f_samples for every output at Xnew (Nt, D): (S, Nt, E) joint samples of the latent functions,
        mean + chol(cov + jitter I) z per output, or (Nt, E) for num_samples=None (pilco_gp_sample_points,
        docs/predict_cov.md).  draws (S, Nt, E): the standard normals to use; None: drawn from `seed` (Philox domain 5; the same
        seed gives the same samples).  full_cov=False: independent draws from the marginals, mean + sqrt(var) z with predict_f's
        mean and variance.  return_parts=True: (samples, dict(mean (Nt, E), cov, chol (E, Nt, Nt), draws)); the draws fed
        back as draws= reproduce the samples bit for bit."""
        return self._predict_f_samples(Xnew, -1, num_samples, full_cov, full_output_cov, seed, draws, jitter, return_parts)

    def _predict_points_jac(self, Xnew, output=-1):
        """(mean, var, dmean, dvar) at Xnew (Nt, D): (Nt, E), (Nt, E) and (Nt, E, D) twice; E = 1 for one output."""
        self._user_factors = None
        self._ensure_factorized()
        mean, var, dmean, dvar = self.ctx.gp_predict_points_jac(
            self._slot, np.asarray(Xnew, np.float64).reshape(-1, self.num_dims), self.num_dims, self.num_outputs, output,
            self._own_inducing())
        return (tensor_value(mean.T), tensor_value(var.T), tensor_value(dmean.transpose(1, 0, 2)),
                tensor_value(dvar.transpose(1, 0, 2)))

    def predict_f_jacobian(self, Xnew):
        """predict_f with the derivatives of mean and latent variance with respect to the input (extension;
        pilco_gp_predict_points_jac, docs/predict_jacobians.md): (mean, var, dmean, dvar), mean and var (Nt, E) with the
        bits of predict_f, dmean[t, e, d] = d mean_e(x_t) / d x_d and dvar likewise, (Nt, E, D)."""
        return self._predict_points_jac(Xnew)

    def predict_y(self, Xnew):
        """predict_f with every output's likelihood variance added to its variance (extension)."""
        mean, var = self._predict_points(Xnew)
        return mean, tensor_value(np.asarray(var) + self.noise.reshape(1, -1))

    # -- reference: mgpr.py:81-89
    def calculate_factorizations(self):
        self._user_factors = None
        self._ensure_factorized()
        return self.ctx.gp_get_factors(self._slot, self.num_outputs)

    # -- reference: mgpr.py:91-149
    def predict_given_factorizations(self, m, s, iK, beta):
        self._sync()
        iK = None if iK is None else np.asarray(iK, np.float64)
        if iK is not None and not np.any(iK):
            iK = None  # 0.0 * iK of the RBF controller (controllers.py:116): skip the stream
        self.ctx.gp_set_factors(self._slot, iK, beta, owner=self)
        self._user_factors = True
        return self.ctx.gp_predict(self._slot, m, s, self.num_dims, self.num_outputs)

    # -- reference: mgpr.py:151-157
    def centralized_input(self, m):
        return self._points() - np.asarray(m, np.float64).reshape(1, -1)

    def K(self, X1, X2=None):
        self._sync()
        return self.ctx.gp_gram(self._slot, X1, X2, self.num_outputs)

    # -- reference: mgpr.py:159-190
    @property
    def Y(self):
        return tensor_value(self._Y)

    @property
    def X(self):
        return tensor_value(self._X)

    @property
    def lengthscales(self):
        return tensor_value(np.stack([np.asarray(m.kernel.lengthscales.numpy(), np.float64).reshape(-1) for m in self.models]))

    @property
    def variance(self):
        return tensor_value(np.array([float(m.kernel.variance.numpy()) for m in self.models]))

    @property
    def noise(self):
        return tensor_value(np.array([float(m.likelihood.variance.numpy()) for m in self.models]))

    @property
    def data(self):
        return (self.X, self.Y)

    @property
    def trainable_parameters(self):
        return [p for p in parameters_of(self.models) if p.trainable]
