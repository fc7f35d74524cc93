// The event predicate of the particle rollouts (particles.hip: k_particle_events) and the refusals of an event table, in one
// place for host and device.  An event (include/pilco_hip.h: pilco_event) is a box over a few state coordinates, or the
// complement of one:
//   inside(x) = every clause holds:  low <= x[dim] && x[dim] <= high     (closed intervals; -inf / +inf: no bound)
//   hit(x)    = complement ? !inside(x) : inside(x)
// A NaN coordinate fails its clause (both comparisons are false): inside is false and hit equals complement.
// Plain C++ apart from the __host__ __device__ marks: tests/test_particle_events_cpu.py compiles this header into a host
// probe and holds the NumPy restatement (tests/helpers/particle_events_restatement.py) to it.
#pragma once
#include "pilco_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PILCO_EVENT_HD __host__ __device__
#else
#define PILCO_EVENT_HD
#endif
namespace pilco {

PILCO_EVENT_HD inline bool event_clause_holds(const pilco_event_clause& c, const double* x) {
    const double v = x[c.dim];
    return c.low <= v && v <= c.high;
}

PILCO_EVENT_HD inline bool event_inside(const pilco_event& ev, const double* x) {
    bool in = true;
    for (int j = 0; j < ev.n_clauses; ++j) in = in && event_clause_holds(ev.clause[j], x);
    return in;
}

PILCO_EVENT_HD inline bool event_hit(const pilco_event& ev, const double* x) {
    const bool in = event_inside(ev, x);
    return ev.complement ? !in : in;
}

// why an event over E state coordinates is refused (nullptr: it is accepted)
PILCO_EVENT_HD inline const char* event_refusal(const pilco_event& ev, int E) {
    if (ev.n_clauses < 1 || ev.n_clauses > PILCO_MAX_EVENT_CLAUSES) return "an event has 1..4 clauses";
    for (int j = 0; j < ev.n_clauses; ++j) {
        const pilco_event_clause& c = ev.clause[j];
        if (c.dim < 0 || c.dim >= E) return "an event clause's dim is outside the state";
        if (c.low != c.low || c.high != c.high) return "an event clause's bound is NaN";
        if (c.low > c.high) return "an event clause has low > high";
    }
    return nullptr;
}

// why a table of events is refused (nullptr: it is accepted); counts: where the counts go
PILCO_EVENT_HD inline const char* event_table_refusal(const pilco_event* events, int n_events, const void* counts, int E) {
    if (n_events < 0 || n_events > PILCO_MAX_EVENTS) return "0..8 events supported";
    if (n_events > 0 && (!events || !counts)) return "events need an event table and counts";
    for (int k = 0; k < n_events; ++k)
        if (const char* why = event_refusal(events[k], E)) return why;
    return nullptr;
}

}  // namespace pilco
