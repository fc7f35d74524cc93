"""NumPy restatement of the events of the particle rollouts (csrc/particle_events.h, k_particle_events in csrc/particles.hip):
the yardstick of tests/test_gpu_particle_events.py, itself held to the header's host probe in
tests/test_particle_events_cpu.py.

An event is dict(clauses=[(dim, low, high), ...], complement=bool); a bound of None is infinite.
  inside(x) = every clause holds, low <= x[dim] and x[dim] <= high (closed; a NaN coordinate fails its clause)
  hit(x)    = not inside(x) if complement else inside(x)
  counts[t, k]    = number of particles p with hit_k(particles[t, p])
  first_hit[p, k] = the smallest t with hit_k(particles[t, p]), or -1

The mutants (MUTANTS) are wrong on purpose: the CPU test asserts that its case table tells every one of them from the
restatement, so a device or host implementation with that mistake could not pass it."""
import numpy as np


def bounds(clause):
    dim, low, high = clause
    return int(dim), (-np.inf if low is None else float(low)), (np.inf if high is None else float(high))


def inside(event, x, closed=True, conj=True):
    """x (..., E) -> bool (...)."""
    x = np.asarray(x, np.float64)
    res = None
    for clause in event["clauses"]:
        dim, low, high = bounds(clause)
        v = x[..., dim]
        with np.errstate(invalid="ignore"):
            ok = ((low <= v) & (v <= high)) if closed else ((low < v) & (v < high))
        res = ok if res is None else ((res & ok) if conj else (res | ok))
    return res


def hit(event, x, closed=True, conj=True, use_complement=True):
    ins = inside(event, x, closed, conj)
    return ~ins if (use_complement and event.get("complement", False)) else ins


def counts(events, particles, **kw):
    """particles (T, P, E) -> (T, K) int64."""
    particles = np.asarray(particles, np.float64)
    out = np.zeros((particles.shape[0], len(events)), np.int64)
    for k, ev in enumerate(events):
        out[:, k] = hit(ev, particles, **kw).sum(axis=1)
    return out


def first_hit(events, particles, keep_first=True, **kw):
    """particles (T, P, E) -> (P, K) int32: the first t with a hit, or -1 (keep_first=False: the mutant that lets a later hit
    overwrite it)."""
    particles = np.asarray(particles, np.float64)
    T, P, _ = particles.shape
    out = np.full((P, len(events)), -1, np.int32)
    for k, ev in enumerate(events):
        h = hit(ev, particles, **kw)   # (T, P)
        for t in range(T):
            sel = h[t] & ((out[:, k] < 0) if keep_first else True)
            out[sel, k] = t
    return out


MUTANTS = {
    "open intervals": dict(closed=False),
    "OR instead of AND": dict(conj=False),
    "complement ignored": dict(use_complement=False),
    "first hit overwritten by a later hit": dict(keep_first=False),
}
