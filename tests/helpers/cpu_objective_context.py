"""A CPU stand-in for the handful of _lib.Context calls the model-fitting glue (pilco_amd/training.py) makes, so that the
HOST side of MGPR.optimize / SMGPR.optimize -- softplus transforms with the 1e-6 noise floor, Gamma priors, packing, one
L-BFGS-B run per output in lockstep, restart draws and bookkeeping -- can be held to the executed reference's end points in
the CPU suite.  TEST INFRASTRUCTURE: the objective values come from oracle/gp_train.py (exact GP) and from the torch restatement
of gpflow's GPRFITC bound in fitc_objective.py; the product computes both on the device (pilco_gp_nlml, pilco_gp_fitc_nlml)."""
import numpy as np
import torch

from helpers.fitc_objective import NotPositiveDefinite, fitc_reference
from oracle import gp_train
from pilco_amd import _lib


class CpuObjectiveContext:
    def __init__(self):
        self._slot_owner = {}
        self.calls = 0

    def gp_set_data(self, slot, X, Y, owner=None):
        self._slot_owner[slot] = owner
        self.X, self.Y = np.array(X, np.float64), np.array(Y, np.float64)

    def gp_set_hyp(self, slot, lengthscales, variance, noise, owner=None):
        self._slot_owner[slot] = owner
        self.ls, self.var, self.nz = np.array(lengthscales, np.float64), np.ravel(variance).astype(np.float64), np.ravel(noise).astype(np.float64)

    def gp_set_inducing(self, slot, Z, owner=None):
        self._slot_owner[slot] = owner

    def gp_nlml(self, slot, D, E, want_grad=True):
        self.calls += 1
        nlml, grad = np.empty(E), np.empty((E, D + 2))
        try:
            for a in range(E):
                nlml[a], grad[a] = gp_train.nlml_and_grad(self.X, self.Y[:, a], self.ls[a], self.var[a], self.nz[a])
        except np.linalg.LinAlgError as exc:
            raise _lib.NotPositiveDefiniteError(3, str(exc))
        return nlml, grad

    def gp_fitc_nlml(self, slot, Z_all, D, E, want_grad=True):
        """gpflow.models.GPRFITC: -log N(y | 0, Qff + diag(Kff - Qff) + noise I) by the inducing-point identities."""
        self.calls += 1
        nthreads = torch.get_num_threads()
        torch.set_num_threads(1)          # bitwise repeatable sums: the fits are hundreds of iterations in a flat valley
        try:
            return self._fitc(Z_all, D, E)
        finally:
            torch.set_num_threads(nthreads)

    def _fitc(self, Z_all, D, E):
        try:
            return fitc_reference(self.X, self.Y, np.asarray(Z_all, np.float64), self.ls, self.var, self.nz)
        except NotPositiveDefinite as exc:
            raise _lib.NotPositiveDefiniteError(3, str(exc))
