// A candidate's view of the model: its interval grid, its migration rates and pulses, the structural checks and status of
// setup_candidate, where it leaves its chain's trunk, and the pair-state record the correction hands from interval to interval.
// Reached by every batch entry and by misti_forward_rates (forward_kernel); restated by tests/exact_forward.py and held by
// tests/test_gpu_exact_forward.py, test_gpu_bounds.py and test_gpu_pulse_times.py.
#pragma once
#include <stdint.h>

#include "misti_device.h"
#include "misti_wave.h"

namespace misti {

// Per-candidate view of the interval grid.  A fractional split time splits
// interval s = floor(st) in two and moves the split index to s+1
// (MigrationInference.__init__, MigrationInference.py:89-99).
struct Grid {
    const double* times;   // [numT0-1]
    const double* lh;      // [numT0][2]
    int numT0;             // intervals of the shared grid
    int numT;              // intervals of this candidate (numT0 or numT0+1)
    int split;             // split index of this candidate
    int ins;               // index of the interval that was split in two, or -1
    double frac;

    __device__ __forceinline__ int src(int t) const { return (ins >= 0 && t > ins) ? t - 1 : t; }
    __device__ __forceinline__ double T(int t) const {
        // t in [0, numT-1)
        if (ins < 0) return times[t];
        if (t < ins) return times[t];
        double whole = times[ins];
        double t1 = frac * whole;
        if (t == ins) return t1;
        if (t == ins + 1) return whole - t1;
        return times[t - 1];
    }
    __device__ __forceinline__ double lhk(int t, int k) const { return lh[2 * src(t) + k]; }
};

// Migration rates / pulse of interval t for this candidate
// (SetModel + MapParameters, MigrationInference.py:229-298).
struct Model {
    const DevModel* m;
    const double* par;     // [n_param] of this candidate
    int split;
    double pv[4];          // the first parameters, cached in registers (a sweep has 1-3)
    const int32_t* bb = nullptr;   // [n_band][2] this candidate's (start, end) of every band, or NULL: the model's
    const int32_t* pt = nullptr;   // [n_pulse] this candidate's pulse times, or NULL: the model's
    __device__ __forceinline__ void cache() { for (int i = 0; i < 4; ++i) pv[i] = (i < m->n_param) ? par[i] : 0.0; }
    __device__ __forceinline__ double param(int i) const {
        return i == 0 ? pv[0] : i == 1 ? pv[1] : i == 2 ? pv[2] : i == 3 ? pv[3] : par[i];
    }
    __device__ __forceinline__ void mig(int t, double& mu0, double& mu1) const {
        mu0 = 0.0; mu1 = 0.0;
        for (int b = 0; b < m->n_band; ++b) {
            const misti_band_t& B = m->bands[b];
            const int start = bb ? bb[2 * b] : B.start;
            int end = bb ? bb[2 * b + 1] : B.end;
            if (end < 0) end = split;
            if (t >= start && t < end) {
                double v = B.param >= 0 ? param(B.param) : B.value;
                if (B.pop == 0) mu0 = v; else mu1 = v;
            }
        }
    }
    __device__ __forceinline__ void pulse(int t, double& pu0, double& pu1) const {
        pu0 = 0.0; pu1 = 0.0;
        for (int b = 0; b < m->n_pulse; ++b) {
            const misti_pulse_t& P = m->pulses[b];
            if (t == (pt ? pt[b] : P.time)) {
                double v = P.param >= 0 ? param(P.param) : P.value;
                if (P.pop == 0) pu0 = v; else pu1 = v;
            }
        }
    }
};

// Per-candidate diagnostics of the correction: overflow guard and work counters.
// Work counters of a chain (last row of the `pr` output).  evals, max_nfev, lm and spec are wave-uniform (scalar registers) and always
// counted; dense, terms and squarings are counted INSIDE the per-lane evaluation and cost three vector registers carried through the
// whole solver loop - exactly what pushed correct_follow_kernel<true> into scratch (10 spilled VGPRs, 44 B; round 4) - so they are
// counted in the diagnostic build only (-DMISTI_WORK_COUNTERS=1: tools/stamp_run.py) and read 0 otherwise.
struct Diag { bool guard = false; int evals = 0, dense = 0, terms = 0, squarings = 0, max_nfev = 0, lm = 0, spec = 0; };

struct PairState { double p[2][3]; };

template <int GROUP = 1>
__device__ __forceinline__ void pulse_pairs(PairState& ps, double pu0, double pu1) {
    double r = pu0 + pu1;                                        // :315-323
    if (uni<GROUP>(!(r > 0))) return;
    int a = pu0 > 0 ? 0 : 1, b = 1 - a;
    for (int k = 0; k < 2; ++k) {
        double pa = ps.p[k][a], pb = ps.p[k][b], pc = ps.p[k][2];
        double omr = 1.0 - r;
        ps.p[k][a] = pa * (omr * omr);
        ps.p[k][b] = pa * (r * r) + pb + pc * r;
        ps.p[k][2] = pa * 2 * omr * r + pc * omr;
    }
}

// ----------------------------------------------------------- the kernels ----
// Candidate structure shared by both kernels: fractional split (:89-99), negative
// parameter guard (:569-572), split beyond the grid.
// SetModel's checks on the bands as this candidate sees them (MigrationInference.py:237-255): start >= sample
// date, start < end (end == -1: the candidate's split index), no overlap within a population.
__device__ __forceinline__ bool bands_valid(const DevModel& m, const int32_t* bb, int split) {
    bool ok = true;
    for (int b = 0; b < m.n_band; ++b) {
        const int sb = bb ? bb[2 * b] : m.bands[b].start;
        int eb = bb ? bb[2 * b + 1] : m.bands[b].end;
        if (eb < -1 || eb > m.numT + 1) ok = false;
        if (eb < 0) eb = split;
        if (sb < m.sample_date || eb <= sb) ok = false;
        for (int c = 0; c < b; ++c) {
            if (m.bands[c].pop != m.bands[b].pop) continue;
            const int sc = bb ? bb[2 * c] : m.bands[c].start;
            int ec = bb ? bb[2 * c + 1] : m.bands[c].end;
            if (ec < 0) ec = split;
            if (sb < ec && sc < eb) ok = false;
        }
    }
    return ok;
}

// SetModel's checks on this candidate's own pulse times (MigrationInference.py:259-279) with the grid bound of validate_model
// (misti_api.cpp): time >= sample date, time < numT + 1, no two pulses at one time.  A time at or beyond the split is valid and
// never applied (the reference's loops run over t < splitT).
__device__ __forceinline__ bool pulses_valid(const DevModel& m, const int32_t* pt) {
    bool ok = true;
    for (int b = 0; b < m.n_pulse; ++b) {
        if (pt[b] < m.sample_date || pt[b] >= m.numT + 1) ok = false;
        for (int c = 0; c < b; ++c) if (pt[c] == pt[b]) ok = false;
    }
    return ok;
}

__device__ __forceinline__ int setup_candidate(const DevModel& m, double st, const double* par, Grid& G, const int32_t* bb = nullptr,
                                               const int32_t* pt = nullptr) {
    int status = MISTI_OK;
    G.times = m.times; G.lh = m.lh; G.numT0 = m.numT;
    double fl = floor(st);
    G.frac = st - fl;
    int s = (int)fl;
    G.ins = -1; G.split = s; G.numT = m.numT;
    if (!(st >= 0) || !(st >= (double)m.sample_date) || s > m.numT) status = MISTI_BAD_STRUCTURE;
    else if (G.frac != 0.0) {
        if (s > m.numT - 2) status = MISTI_BAD_STRUCTURE;
        else { G.ins = s; G.split = s + 1; G.numT = m.numT + 1; }
    }
    if (status == MISTI_OK && m.n_band > 0 && !bands_valid(m, bb, G.split)) status = MISTI_BAD_STRUCTURE;
    if (status == MISTI_OK && pt && !pulses_valid(m, pt)) status = MISTI_BAD_STRUCTURE;
    // construction errors (PrintError + exit in the reference's __init__/SetModel) come before the guard of JAFSLikelihood (:569-572)
    if (status == MISTI_OK) for (int i = 0; i < m.n_param; ++i) if (par[i] < 0) status = MISTI_NEG_PARAM;
    if (status == MISTI_OK && G.split >= G.numT) status = MISTI_INF_COAL;
    return status;
}

// First interval whose rates depend on THIS candidate's split - where it leaves the trunk of its chain: the start of the
// smoothing run (of either genome) that the split cuts, or the shortened interval of a fractional split.  Used by the candidate
// kernel (where to start from) and by setup_kernel (from which interval on the chain's trunk has to store records).
__device__ __forceinline__ int trunk_leave(const DevModel& m, const Grid& G) {
    int t_own = (G.ins >= 0) ? G.ins : G.split;
    if (m.flags & MISTI_SMOOTH) {
        if (G.ins >= 0) {
            t_own = min(m.run_start[G.ins], m.run_start[m.numT + G.ins]);
        } else if (G.split > 0) {
            for (int k = 0; k < 2; ++k)
                if (m.run_end[k * m.numT + G.split - 1] > G.split) t_own = min(t_own, m.run_start[k * m.numT + G.split - 1]);
        }
    }
    return t_own;
}

}  // namespace misti
