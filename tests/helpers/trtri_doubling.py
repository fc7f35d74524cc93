"""NumPy restatement of launch_trtri's recursive doubling on NB x NB blocks (float64): the order in which the device forms
L^-1.  Shared by tests/test_factorisations_cpu.py (the sensitivity of the GPU criteria) and
tests/helpers/predict_edges_reference.py (the device-ordered restatement of the posterior)."""
import os
import re

import numpy as np
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def header_const(name):
    src = open(os.path.join(ROOT, "pilco_amd", "csrc", "common.h")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


NB = header_const("NB")


def pad(n):
    return -(-n // NB) * NB


def trtri_levels(npad):
    """launch_trtri's sub-problems per level: (h, nsub, rows of the last sub-problem's lower half)."""
    out, h = [], NB
    while h < npad:
        nsub = (npad - h + 2 * h - 1) // (2 * h)
        out.append((h, nsub, (npad - h) - (nsub - 1) * 2 * h))
        h *= 2
    return out


def doubling(L, drop_clipped=False, perturb=None):
    """L^{-1} by launch_trtri's recursive doubling on 64 x 64 blocks (float64).  drop_clipped: the last, clipped
    sub-problem of the top level is skipped; perturb=(I, J, rel): tile (I, J) of the result scaled by 1 + rel."""
    npad = L.shape[0]
    X = np.zeros_like(L)
    for b in range(0, npad, NB):
        X[b:b + NB, b:b + NB] = sla.solve_triangular(L[b:b + NB, b:b + NB], np.eye(NB), lower=True)
    for h, nsub, _ in trtri_levels(npad):
        for q in range(nsub):
            a0, b0 = q * 2 * h, q * 2 * h + h
            b1 = min(b0 + h, npad)
            if drop_clipped and h == trtri_levels(npad)[-1][0] and q == nsub - 1 and b1 - b0 < h:
                continue
            T = L[b0:b1, a0:b0] @ X[a0:b0, a0:b0]
            X[b0:b1, a0:b0] = -X[b0:b1, b0:b1] @ T
    if perturb:
        I, J, rel = perturb
        X[I * NB:(I + 1) * NB, J * NB:(J + 1) * NB] *= 1 + rel
    return X


def padded_inverse(L):
    """L^-1 (n, n) of a lower-triangular factor by the device's route: padded to a multiple of NB with a unit diagonal."""
    n = L.shape[0]
    P = np.eye(pad(n))
    P[:n, :n] = L
    return doubling(P)[:n, :n]
