// Shared between the kernels (misti_kernels.hip and its headers) and the C-ABI host layer (misti_api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/misti_hip.h"

#include "misti_consts.h"

namespace misti {

// Per-row view of the constant chain structure, in __constant__ memory.
struct DevTables {
    int src[MAXNZ][64];      // source state of the n-th off-diagonal entry of row `lane`
    int kind[MAXNZ][64];     // 0 la0, 1 la1, 2 mu0, 3 mu1
    int mult[MAXNZ][64];     // integer multiplicity
    int dcnt[4][64];         // exit-rate multiplicities of the state (diagonal = -sum dcnt*rate)
    int jaf[7][64];          // class-major StateToJAF
    int jaf1[7][NS1];
    unsigned long long jaf_bits[7][3];   // the same weights (0..7) as bit planes over the 44 states: one 24-byte load per class
    unsigned int jaf1_bits[7];           // one-population weights, 3 bits per state
    int grp_lo[NS1], grp_hi[NS1];
    int anc_n[2], anc_dst[2], anc_src[2][8];
    int pulse_n[2][64];
    int pulse_src[2][64][MAXPULSE];
    int pulse_ab[2][64][MAXPULSE];
    double tal_zr[TALBOT_HALF], tal_zi[TALBOT_HALF];   // Talbot nodes z_k (upper half plane)
    double tal_cr[TALBOT_HALF], tal_ci[TALBOT_HALF];   // weights c_k = (i/N) exp(z_k) z'(theta_k)
};

// Kernel-argument copy of the model (device pointers).
struct DevModel {
    int numT;
    int sample_date;
    unsigned flags;
    int n_band, n_pulse, n_param;
    double mixture_th;
    const double* times;     // [numT-1]
    const double* lh;        // [numT][2]
    const int* run_start;    // [2][numT]  smoothing runs of constant lh (MigrationInference.py:387-405)
    const int* run_end;      // [2][numT]
    const int* leave_ok;     // [numT]     1 where SOME split (integer or fractional) leaves a chain's trunk (trunk_leave): the only intervals
                             //            whose trunk record a candidate can ever read
    misti_band_t bands[MISTI_MAX_BANDS];
    misti_pulse_t pulses[MISTI_MAX_PULSES];
};

// Device buffers of the chain machinery (see correct_kernel).  Candidates with bitwise identical
// parameter vectors share a chain; chains are found by inserting every candidate into an open-addressing
// table keyed by its parameters (discover_kernel): the first one in a slot owns the chain.
struct ChainBufs {
    int32_t* n_chains;      // [4]: chains; candidate blocks of setup_kernel that have finished; head of the chain queue; spare
    int32_t* z_n_chains;    // the OTHER set of {n_chains, table, slot_len, slot_keep}: cleared by this batch for the next one
    int32_t* z_table;
    int32_t* z_slot_len;
    int32_t* z_slot_keep;
    int32_t* table;         // [tsize] slot -> owner candidate + 1, 0 = empty
    int32_t* slot_chain;    // [tsize] slot -> chain
    int32_t* slot_len;      // [tsize] slot -> number of full intervals needed (max over members)
    int32_t* slot_keep;     // [tsize] slot -> numT - (first interval at which a member leaves the trunk), max over members: the trunk
                            //         stores its records from interval numT - slot_keep on (0: no member reads any)
    int32_t* resume_t;      // [n] per chain that yielded in a packed launch: the interval it resumes at (correct_resume_kernel)
    int32_t* resume_list;   // [n] those chains; length n_chains[3], head n_chains[2]
    int32_t* chain_order;   // [n] chains by descending length (the last candidate block of setup_kernel sorts them): dispatch order
    int32_t* slot_of;       // [n] candidate -> slot
    int32_t* of;            // [n] candidate -> chain, resolved by the idle blocks of the chain launch
    int32_t* chain_slot;    // [n] chain -> slot
    int32_t* rep;           // [n] chain -> a member candidate (its parameters)
    uint32_t tmask;         // tsize - 1 (tsize a power of two >= 2 n)
    double* lc;             // [n][numT][2]     per chain: corrected rates, unsmoothed
    double* trace;          // [n][numT+1][6]   per chain: pair state before interval t (.Pr layout)
    int32_t* fail_t;        // [n] per chain: first failing interval, INT_MAX if none
    int32_t* fail_status;   // [n]
    double* work;           // [n][6] per chain: work counters
    double* tail_lc;        // [n][2] per candidate with a fractional split
    double* tail_state;     // [n][6]
    int32_t* tail_status;   // [n]
    double* trunk;          // [trunk_cap][numT][TRUNK_REC] per chain: 44-state vector + occupation integrals before interval t
    int32_t* trunk_ok;      // [trunk_cap] per chain: last valid record
    int64_t trunk_cap;      // chains the trunk buffer holds (0: no trunk)
    int32_t* simd_load;     // [PAIR_TABLE] chain waves resident per (compute unit, SIMD) - all contexts of the device share it - or NULL (correct_follow_kernel)
    int32_t* hint;          // host-pinned [3] or NULL: {chains, candidates, batch tag}, written by the last block of discover_kernel
    int32_t seq;            // this batch's tag
    int32_t unsorted;       // the caller knows its batch has one split time: bit 0 - candidates are dispatched in their own order, bit 1 - chains in
                            // order of arrival (setup_kernel sorts neither)
    int32_t integer_splits; // the caller (or the host-buffer entry point, which sees them) says no split time has a fractional part: no tail launch was
                            // made, and a candidate that has one after all is refused (spectrum_kernel)
    const int32_t* bounds;  // [n][n_band][2] per-candidate (start, end) of every band, or NULL: the model's
    const int32_t* pulse_times;   // [n][n_pulse] per-candidate time of every pulse, or NULL: the model's
    double* post_lam;       // [n][numT+1] default fit: rates after the split (postsplit_kernel -> spectrum kernel)
    int32_t* post_word;     // [n][numT+1] their solver words, or NULL (trace off)
    // solver trace (misti_enable_solver_trace), all NULL when off
    int32_t* solver;        // [n][numT] per chain: packed word of interval t (nfev | status << 16 | kind << 20)
    int32_t* tail_solver;   // [n] per candidate with a fractional split: the shortened interval
    int32_t* cand_solver;   // [n][numT+1] per candidate, assembled by the spectrum kernel (+ post-split solves)
    double* iters;          // [iter_cap][numT][MISTI_TRACE_MAX_ITER][2] trial points of the unbounded solves, or NULL
    int64_t iter_cap;       // chains the iterate buffer holds
};

__host__ __device__ __forceinline__ int32_t solver_word(int nfev, int status, int kind) {
    return (int32_t)((nfev & 0xffff) | ((status & 15) << 16) | ((kind & 15) << 20));
}

__device__ __forceinline__ int64_t chain_of(const ChainBufs& cb, int64_t cand) { return cb.of[cand]; }
__device__ __forceinline__ int chain_len(const ChainBufs& cb, int64_t ch) { return cb.slot_len[cb.chain_slot[ch]]; }

// What the searches (misti_nm.hip, misti_de.hip, misti_ens.hip) share on the device.
// -JAFSLikelihood as an optimiser sees it; no value = +inf
__device__ __forceinline__ double objective(double llk) { return (llk == llk && llk > -INFINITY) ? -llk : INFINITY; }
// the value as rounded so far: opaque to the optimiser, so a product passed through it is never contracted into an fma
__device__ __forceinline__ double rn(double v) { __asm__ volatile("" : "+v"(v)); return v; }
// numpy.clip(x, lo, hi) = minimum(maximum(x, lo), hi) on one coordinate: a NaN passes through (fmin / fmax would drop it), an x equal to
// a bound comes back as the bound itself (a zero takes the bound's sign, as NumPy's does), +-inf bounds never bind.  lo <= hi, neither NaN.
__device__ __forceinline__ double box_clip(double x, double lo, double hi) {
    double t = x > lo ? x : lo;
    t = t < hi ? t : hi;
    return x != x ? x : t;
}

// Batched Nelder-Mead (misti_nm.hip): everything a start owns, in HBM.  V = N + 1 vertices.
enum { NM_NONE = 0, NM_REFLECT = 1, NM_EXPAND = 2, NM_CONTRACT = 3, NM_INSIDE = 4,
       NM_CUT = 5 };        // the evaluation budget (maxfev) ran out before the iteration's second point: SciPy abandons the iteration there
// One engine batch of the search: what each of its slots hands the engine.  Everything a start passes on to its points beyond their
// coordinates is a field here - and nowhere else.  The five batches' arrays of one kind are one contiguous block, in the order of the
// enum below (the host clears a kind with one memset).
struct NmBatch {
    double* pts;            // [slots][N]      the points
    double* split;          // [slots]         their split times (negative: no point in this slot)
    int32_t* row;           // [slots]         their replicate rows (NULL unless row_of is set; empty slots carry row 0)
    int32_t* bnd;           // [slots][nb2]    their band bounds (NULL unless bounds_of is set; empty slots carry zeros)
    int32_t* put;           // [slots][np]     their pulse times (NULL unless pulses_of is set; empty slots carry zeros)
    double* par;            // [slots][N - 1]  the engine's parameter vectors (fit_split only; NULL otherwise, and for a model without a
                            //                 parameter: N == 1, the array has no width)
};
// What a search hands its points beyond their coordinates: start (or search) s of Nelder-Mead, differential evolution and the ensemble
// sampler alike.  A per-start field is added HERE (and to put_point / put_none below, and to RowsProblem on the host) - nowhere else.
struct PointSource {
    int N;                  // coordinates of a point
    double split;           // the split time every point is evaluated at (unless split_of is set; MISTI_SPLIT_ONE only, 0 otherwise)
    const double* split_of; // [S] or NULL: the split time of each start's points (misti_nm_solve_rows); NULL: `split` for all
    const int32_t* row_of;  // [S] or NULL: the replicate row of each start's points; set together with split_of
    const int32_t* bounds_of;   // [S][nb2] or NULL: the band bounds of each start's points (misti_nm_solve_bounds); only with row_of
    int nb2;                // 2 n_band: int32 per bound set (bounds_of set)
    const int32_t* pulses_of;   // [S][np] or NULL: the pulse times of each start's points (misti_nm_solve_pulses); only with row_of
    int np;                 // n_pulse: int32 per pulse-time set (pulses_of set)
    int fit_split;          // 1 (misti_nm_solve_split; only with row_of): the LAST of the N coordinates is the point's split time and the first
                            // N - 1 are the model's parameters - every point laid out for a batch leaves its split in the slot's split and its
                            // parameters in the batch's compact `par`, which the engine reads instead of the points.  0: nothing of this is
                            // written or read
    // The box (misti_nm_solve_box / misti_basinhopping_box): SciPy's Nelder-Mead with bounds=Bounds(lo, hi).  Every point the search lays
    // out is clipped to [lo, hi] per coordinate before put_point() reads it, a fitted split (coordinate N - 1) like any other.  Both NULL:
    // no box - nothing of it is allocated, read or written, and a kernel branches on it by one wave-uniform pointer test.  The population
    // searches always have one: finite, lo <= hi.
    const double* box_lo;   // [N], or [S][N] with box_per_start; NULL: no box
    const double* box_hi;   // the same shape; NULL together with box_lo
    int box_per_start;      // 1: start s has its own box, rows s of the two arrays; 0: one box for every start
    const uint64_t* ids;    // [S] or NULL: the random stream of search s is Philox(key=[seed, ids[s]]); NULL: ids[s] = s
};
// where start s's box begins in box_lo / box_hi, and the id of its random stream
__device__ __forceinline__ int64_t box_of(const PointSource& src, int64_t s) { return src.box_per_start ? s * src.N : 0; }
__device__ __forceinline__ uint64_t id_of(const PointSource& src, int64_t s) { return src.ids ? src.ids[s] : (uint64_t)s; }
// What a slot of a batch hands the engine beside its point.  put_point: slot j of batch b carries start s's point pt (the slot's entry
// of b.pts, already written) - the start's split time, replicate row, band bounds and pulse times: one split for all starts (misti_nm_solve), or per
// start (misti_nm_solve_rows: row_of set; misti_nm_solve_bounds: bounds_of as well; misti_nm_solve_pulses: pulses_of).  With the split
// as a coordinate (misti_nm_solve_split, fit_split) the split is the point's own last coordinate and the coordinates before it go to
// the compact parameter array the engine reads.  Arrays of a path that is not taken are NULL and nothing is written to them.
__device__ __forceinline__ void put_point(const PointSource& src, const NmBatch& b, int64_t j, int64_t s, const double* pt) {
    const int P = src.N - 1;
    b.split[j] = src.split_of ? src.split_of[s] : src.split;
    if (src.row_of) b.row[j] = src.row_of[s];
    if (src.bounds_of) for (int k = 0; k < src.nb2; ++k) b.bnd[j * src.nb2 + k] = src.bounds_of[s * src.nb2 + k];
    if (src.pulses_of) for (int k = 0; k < src.np; ++k) b.put[j * src.np + k] = src.pulses_of[s * src.np + k];
    if (src.fit_split) { b.split[j] = pt[P]; for (int k = 0; k < P; ++k) b.par[j * P + k] = pt[k]; }
}
// put_none: slot j carries no point (a start that needs none in this phase) - a negative split, row 0, all-zero bounds, pulse times and
// parameters, a zeroed point: no row index ever leaves the table, and a negative split is refused (setup_candidate) before any bound or
// time of its slot is read.  pt: the slot's entry of b.pts, or NULL for a slot that has no START either: such a slot keeps whatever
// point and parameters it held.
__device__ __forceinline__ void put_none(const PointSource& src, const NmBatch& b, int64_t j, double* pt) {
    const int P = src.N - 1;
    b.split[j] = -1.0;
    if (src.row_of) b.row[j] = 0;
    if (src.bounds_of) for (int k = 0; k < src.nb2; ++k) b.bnd[j * src.nb2 + k] = 0;
    if (src.pulses_of) for (int k = 0; k < src.np; ++k) b.put[j * src.np + k] = 0;
    if (!pt) return;
    for (int k = 0; k < src.N; ++k) pt[k] = 0.0;
    if (src.fit_split) for (int k = 0; k < P; ++k) b.par[j * P + k] = 0.0;
}
// The batches of a search and their slots: the initial simplices [S * V] (pts is `sim` itself); per iteration, live starts compacted,
// the reflection points [S], the expansion / contraction points [S] and the shrunk vertices [S * N]; or, speculative iterations (few
// live starts: latency-bound), every point SciPy COULD ask for in the iteration as one batch [spec_cap * (4 + N)]: per live start the
// reflection, expansion, outside / inside contraction and the N shrunk vertices.
enum { NM_B_INIT, NM_B_REFLECT, NM_B_SECOND, NM_B_SHRINK, NM_B_SPEC, NM_BATCHES };
struct NmState {
    int64_t S;              // starts
    int N;                  // parameters
    int maxiter;
    int64_t maxfun;
    double xatol, fatol;
    PointSource src;        // what a start hands its points
    // per start
    double* sim;            // [S][V][N] simplices, best vertex first after every sort
    double* fsim;           // [S][V]    objective (-llk, +inf where the engine has no value)
    double* scratch;        // [S][V][N] row permutation buffer of the sort
    double* fxr;            // [S]
    int32_t* nit;           // [S] SciPy's `iterations`
    int32_t* nfev;          // [S] SciPy's fcalls
    int32_t* done;          // [S] -1 while running; 0 converged, 1 evaluation budget, 2 iteration budget
    int32_t* kind;          // [S] NM_* of the iteration in progress
    int32_t* shrunk;        // [S] 0: no shrink in the iteration in progress; 1 + n: a shrink of which n vertices were evaluated (n < N: the budget
                            //     ran out inside it - vertex n + 1 is moved but keeps its old value, the rest is untouched, as in SciPy)
    NmBatch b[NM_BATCHES];  // per slot of the batches; the kernels index it with constants only (a by-value argument stays in registers)
    int64_t spec_cap;       // live starts up to which an iteration is speculative
    int32_t* idx_cur;       // [S] slot -> start of the iteration in progress (read only; the next iteration's idx_next)
    int32_t* count_cur;     // [1] its number of live starts
    int32_t* idx_next;      // [S] slot -> start of the next iteration (filled by the kernel that ends this one)
    int32_t* count_next;    // [1]
};
hipError_t launch_nm_init(const NmState& st, const double* starts, hipStream_t stream);
hipError_t launch_nm_begin(const NmState& st, const double* llk0, hipStream_t stream);
hipError_t launch_nm_reflect(const NmState& st, int64_t bound, const double* llk1, hipStream_t stream);
hipError_t launch_nm_accept(const NmState& st, int64_t bound, const double* llk2, hipStream_t stream);
hipError_t launch_nm_finish(const NmState& st, int64_t bound, const double* llk3, hipStream_t stream);
hipError_t launch_nm_result(const NmState& st, double* x, double* llh, int32_t* status, hipStream_t stream);
hipError_t launch_nm_spec_points(const NmState& st, int64_t bound, hipStream_t stream);
hipError_t launch_nm_spec_step(const NmState& st, int64_t bound, const double* llk, int32_t* live_host, hipStream_t stream);
hipError_t launch_nm_spec_finish(const NmState& st, int64_t bound, const double* llk, hipStream_t stream);

// Batched basin hopping (scipy.optimize.basinhopping with Nelder-Mead as the local minimiser; reference semantics
// MigrationInference.Solve(globalOpt=True), /root/reference/MigrationInference.py:723-725): everything a start owns besides its simplex.
struct BhState {
    int64_t S;
    int N;
    double beta;            // 1 / T (inf for T == 0), Metropolis
    double target, factor;  // AdaptiveStepsize: target acceptance rate, stepwise factor
    int interval;
    double* x_cur;          // [S][N] incumbent
    double* f_cur;          // [S]
    int32_t* ok_cur;        // [S]    success of the incumbent's minimisation
    double* x_best;         // [S][N] Storage: lowest successful result
    double* f_best;         // [S]
    int32_t* ok_best;       // [S]
    double* stepsize;       // [S]
    int32_t* nstep;         // [S]    AdaptiveStepsize.nstep (reset at every adjustment)
    int32_t* naccept;       // [S]
    int32_t* nfev;          // [S]    res.nfev: evaluations of all minimisations
    int32_t* failures;      // [S]    res.minimization_failures
    int32_t* accepted;      // [S]    hops accepted (not a SciPy field; diagnostics)
};
// after a minimisation from `trial` (results in x_min / llh_min / nm.nfev / nm status): initial one (hop < 0) or hop `hop` with its Metropolis draw
hipError_t launch_bh_update(const BhState& bh, const NmState& nm, const double* x_min, const double* llh_min, const int32_t* nm_status,
                            int hop, int niter, const double* uniforms, hipStream_t stream);
// next trial points: AdaptiveStepsize.take_step + RandomDisplacement with the pre-drawn uniforms of hop `hop`
hipError_t launch_bh_step(const BhState& bh, int hop, int niter, const double* uniforms, double* trial, hipStream_t stream);
hipError_t launch_bh_result(const BhState& bh, double* x, double* llh, hipStream_t stream);

// Differential evolution per search (misti_de.hip; the rule is optimize.differential_evolution_rule, operation for operation):
// everything a search owns, in HBM.  A generation of every live search is ONE engine batch of P points per search; batch slot
// j * P + i carries member i of the search in live slot j.  What a search hands its points (split, row, bounds, pulse times, the box, its id) is a
// PointSource, and the batch is an NmBatch: the engine sees what a Nelder-Mead batch hands it.
struct DeState {
    int64_t S;              // searches
    int N, P;               // coordinates, members
    int maxiter;            // generations
    double tol, atol;       // stop: var(f) <= (atol + tol |mean(f)|)^2 over members that all have a value
    double F_lo, F_hi, CR;
    uint64_t seed;
    PointSource src;        // what a search hands its points; always with rows and a finite box
    double* pop;            // [S][P][N] the population
    double* f;              // [S][P]    its objective (-llk, +inf where the engine has no value)
    int32_t* best;          // [S] the member with the lowest objective (ties: the lowest index)
    int32_t* nit;           // [S] generations completed
    int32_t* done;          // [S] -1 while running; 0 converged, 2 generation budget
    NmBatch b;              // [S * P] slots: the initial population, then every generation's trial points (live searches compacted)
    int32_t* idx_cur;       // [S] live slot -> search of the generation in progress
    int32_t* count_cur;     // [1]
    int32_t* idx_next;      // [S] filled by the selection that ends the generation
    int32_t* count_next;    // [1]
    unsigned long long* points;   // [1] points handed to the engine that carry a search's point (empty slots not counted)
};
hipError_t launch_de_init(const DeState& st, const double* starts, hipStream_t stream);
// trial points of generation `gen` (>= 1) for the first `bound` live slots (slots beyond the live searches carry no point)
hipError_t launch_de_trial(const DeState& st, int64_t bound, int gen, hipStream_t stream);
// values of generation `gen` are in (gen 0: the initial population, every search live in its own slot): selection, best, stop test,
// and the searches that go on compacted into idx_next / count_next
hipError_t launch_de_select(const DeState& st, int64_t bound, int gen, const double* llk, hipStream_t stream);
// x[S][N], llh[S], nit / nfev / status[S]; pop_llh[S][P] (or NULL): -f
hipError_t launch_de_result(const DeState& st, double* x, double* llh, int32_t* nfev, int32_t* status, double* pop_llh, hipStream_t stream);

// The prior of misti_ensemble_sample_prior / misti_tempered_sample_prior (misti_prior.h), per coordinate of a search or fit.  All NULL
// for the entries without one: nothing of it is allocated, read or written, and a kernel branches on it by one wave-uniform pointer
// test (`kind`), as on PointSource's box.
struct EnsPrior {
    const int32_t* scale;   // [N], or [S / L][N] with per_start: MISTI_COORD_*
    const int32_t* kind;    // the same shape: MISTI_PRIOR_*; NULL: no prior
    const double* p0;       // the same shape
    const double* p1;
    int per_start;
    double* y;              // [S * H][N] the sampling coordinates of the slot's proposal: with a prior the slot's `pts` holds the natural point
};
__device__ __forceinline__ int64_t prior_of(const EnsPrior& pr, int64_t fit, int N) { return pr.per_start ? fit * N : 0; }

// Ensemble sampler per search (misti_ens.hip; the rule is optimize.ensemble_rule, operation for operation): everything a search
// owns, in HBM.  A half-step of every search is ONE engine batch of H = W / 2 points per search; batch slot s * H + m carries the
// proposal of walker half * H + m of search s (the initial ensemble: slot s * W + i, walker i).  No search ever stops, so slots are
// never compacted.  What a search hands its points is a PointSource, and the batch is an NmBatch.
//
// The tempered sampler (misti_pt.hip) runs the L rungs of its fits through the same kernels as S = fits x L searches: search s is rung
// s % L of fit s / L.  Row, split, bounds, pulse times, box and stream id are the FIT's (src is indexed by s / L), the temperature is
// the rung's (temp[(fit or 0) L + l]), the step handed to ens_draw is step L + l, and the chain keeps the coordinates of rung 0 only
// ([fits][n_keep][W][N]) beside the values of every rung ([S][n_keep][W]).  L = 1 is misti_ensemble_sample.
struct EnsState {
    int64_t S;              // searches
    int L = 1;              // rungs per fit: S is a multiple of it
    int N, W;               // coordinates, walkers (even)
    int thin;               // the ensemble after steps thin, 2 thin, ... is kept
    double a, am1;          // the stretch's scale and a - 1 as rounded once
    uint64_t seed;
    const double* temp;     // [L], or [S / L][L] with temp_per_start
    int temp_per_start;
    PointSource src;        // what a search hands its points; always with rows and a finite box
    EnsPrior prior;         // all NULL without a prior
    double* x;              // [S][W][N] the ensemble (with a prior: in sampling coordinates)
    double* llh;            // [S][W]    its log-likelihood (-inf where the engine has no value)
    double* z;              // [S * H]   the stretch of the slot's proposal; negative: rejected in advance, the slot carries no point
    double* u_acc;          // [S * H]   the decision's uniform
    int32_t* accepted;      // [S][W]    proposals accepted, per walker: plain stores by the walker's own thread
    int32_t* submitted;     // [S][W]    proposals of the walker handed to the engine (those rejected in advance are not)
    NmBatch b;              // [S * W] slots
    double* chain;          // [S / L][n_keep][W][N] or NULL: rung 0 of every fit
    double* chain_llh;      // [S][n_keep][W] or NULL
    int64_t n_keep;
    long long* points;      // [S] the sum of `submitted` over the walkers of a search (ens_result_kernel); the host adds the searches
};
hipError_t launch_ens_init(const EnsState& st, const double* init, hipStream_t stream);
// proposals of half `half` (0, 1) of step `step` (>= 1)
hipError_t launch_ens_propose(const EnsState& st, int64_t step, int half, hipStream_t stream);
// values are in.  half < 0: the initial ensemble's; otherwise the decisions of that half-step, and behind half 1 of a kept step the
// ensemble's row of the chain
hipError_t launch_ens_accept(const EnsState& st, int64_t step, int half, const double* llk, hipStream_t stream);
hipError_t launch_ens_result(const EnsState& st, hipStream_t stream);

// Tempered ensemble sampler (misti_pt.hip; the rule is optimize.tempered_rule, operation for operation): what the swap rounds and the
// reduction add to an EnsState with L rungs.
struct PtState {
    int32_t* swap_proposed; // [fits][L - 1] pairs in which both walkers had a value
    int32_t* swap_accepted; // [fits][L - 1] pairs that traded places
};
// the swap round behind half 1 of step `step`: pairs (l, l + 1) for l = first, first + 2, ... < L - 1; the caller launches it only where
// there is such a pair
hipError_t launch_pt_swap(const EnsState& st, const PtState& pt, int64_t step, int first, hipStream_t stream);
// rung_llh[fits][L] and logz[fits] from st.chain_llh over the kept steps burn ... n_keep - 1
hipError_t launch_pt_reduce(const EnsState& st, int64_t burn, double* rung_llh, double* logz, hipStream_t stream);

// Replicate epilogue fused into the spectrum kernel up to this many replicates (one launch less per batch).
constexpr int LLK_INLINE_MAX = 8;

hipError_t upload_tables(const DevTables& t);
size_t spectrum_lds_bytes(int numT, int wpb);
// Diagnostic overrides of the launch shape, read from the environment ONCE per context (misti_create) - never on the batch path.
struct Tuning {
    int chains_per_wave = 0;   // MISTI_CHAINS_PER_WAVE: 1 | 2 | 4 | 8 | 10 forces the packing of the chain launch
    int cands_per_wave = 0;    // MISTI_CANDS_PER_WAVE: ... of the packed kernels (chains and tails)
    bool no_follow = false;    // MISTI_NO_FOLLOW=1: trunks in the launch after the chains
    bool no_trunk = false;     // MISTI_NO_TRUNK=1: every candidate walks all its intervals
    int follow_max = 0;        // MISTI_FOLLOW_MAX_CHAINS: chains up to which a batch runs one chain per wave (0: FOLLOW_MAX_CHAINS)
    int min_blocks = 0;        // MISTI_FOLLOW_MIN_BLOCKS: least workgroups of that launch (0: FOLLOW_MIN_BLOCKS)
    int yield_nfev = -1;       // MISTI_YIELD_NFEV: evaluations after which a solve of a PACKED launch yields its chain to correct_resume_kernel
                               // (-1: YIELD_NFEV; 0: never)
    bool two_phase = true;     // MISTI_TWO_PHASE=0: everything behind a yielding packed launch on one stream (no phase-1 launch beside the resume launch)
    bool pairing = true;       // MISTI_FOLLOW_PAIRING=0: the chain always on the first wave of its workgroup (default: placement-aware, correct_follow_kernel)
    int k2_single_waves = -1;  // MISTI_K2_SINGLE_WAVES: 1 / 0 forces kernel 2's workgroups to one / four waves (-1: chosen per batch, run_dev)
    int busy_contexts = -1;    // MISTI_FOLLOW_BUSY_CONTEXTS: other contexts with a batch in flight from which on a batch of more than
                               // FOLLOW_BUSY_CHAINS chains is packed (-1: FOLLOW_BUSY_CONTEXTS; 0: never look, always the latency shape)
    int scan_slices = 0;       // MISTI_SCAN_SLICES: forces the number of candidate slices of misti_scan_best_dev / misti_scan_profile_dev (0: scan_best_slices' / scan_profile_slices' choice)
};
Tuning read_tuning();
int64_t trunk_capacity(int64_t n_cand, const Tuning& tn);
uint32_t chain_table_size(int64_t n_cand);
hipError_t launch_setup(const DevModel& m, int64_t n, const double* params, const double* split, const ChainBufs& cb, int32_t* order,
                        int64_t n_rep, const double* jsfs, double* consts, int unfolded, hipStream_t stream);
int correct_cands_per_wave(int64_t n_items, const Tuning& tn);
bool trunk_follows(int cpw_chains, int64_t trunk_cap, const Tuning& tn);
hipError_t launch_correct(const DevModel& m, int64_t n_cand, const ChainBufs& cb, const double* split, const double* params,
                          int cpw, bool follow, int64_t est_chains, const Tuning& tn, int yield_nfev, hipStream_t stream, hipEvent_t after_packed = nullptr);
hipError_t launch_spectrum(const DevModel& m, int64_t n_cand, const int32_t* order, const double* split, const double* params,
                           const ChainBufs& cb, double* lc_out, double* pr_out, double* jafs, int32_t* status, double* diag,
                           int64_t n_rep, const double* jsfs, const double* consts, double* llk, bool follow, bool skip_post, bool single_waves, const Tuning& tn, hipStream_t stream,
                           int phase = 0);
hipError_t launch_forward(const DevModel& m, int64_t n_cand, const double* split, const double* params, int hold_mu, double* lh_out, double* pr_out,
                          int32_t* status, hipStream_t stream);
// misti_pair_residuals: problems[n][10] -> out[n][4], one problem per lane through pair_eval<cpfit>
hipError_t launch_pair_residuals(bool cpfit, int64_t n, const double* problems, double* out, hipStream_t stream);
// misti_lsq_probe: problems[n][MISTI_LSQ_IN] -> out[n][MISTI_LSQ_OUT], one problem per lane through the solver's linear algebra
hipError_t launch_lsq_probe(int kind, int64_t n, const double* problems, double* out, hipStream_t stream);
hipError_t launch_argmax(int64_t n_cand, int64_t n_rep, const double* llk, int32_t* best, double* best_llk, hipStream_t stream);
// The k best candidates per replicate without the table (misti_scan_best_dev): llk_kernel's values reduced where they are computed.
// `slices` = scan_best_slices(...) lists of width scan_best_width(k) go through part_v / part_i ([slices][width][n_rep] each), then one
// merge launch writes best[n_rep][k] / best_llk[n_rep][k] (NULL: not wanted).  n_cand == 0 (slices == 0): -1 / -inf everywhere.
int scan_best_width(int k);
int64_t scan_best_slices(int64_t n_cand, int64_t n_rep, const Tuning& tn);
hipError_t launch_scan_best(int64_t n_cand, const double* jafs, const int32_t* status, int64_t n_rep, const double* jsfs, const double* consts,
                            int k, int32_t* best, double* best_llk, int64_t slices, double* part_v, int32_t* part_i, int unfolded, hipStream_t stream);
// The profile per group and replicate without the table (misti_scan_profile_dev): per (replicate, group) the best candidate of the
// group, llk_kernel's values under the scan's total order.  `index` (scan_profile_index_size(...) integers: first [n_group + 1],
// cursor [n_group], members [n_cand]) is the group index, built on the device: count, exclusive scan, scatter; `slices` =
// scan_profile_slices(...) pairs per (group, replicate) go through part_v / part_i ([slices][n_group][n_rep] each), then one merge
// launch writes prof_llk[n_rep][n_group] / prof_best (NULL: not wanted).  n_cand == 0 (slices == 0): -inf / -1 everywhere; index,
// part_v and part_i may then be NULL and only the outputs are touched.
int64_t scan_profile_slices(int64_t n_cand, int64_t n_group, int64_t n_rep, const Tuning& tn);
size_t scan_profile_index_size(int64_t n_cand, int64_t n_group);
hipError_t launch_scan_profile(int64_t n_cand, const double* jafs, const int32_t* status, const int32_t* group, int32_t n_group,
                               int64_t n_rep, const double* jsfs, const double* consts, double* prof_llk, int32_t* prof_best,
                               int64_t slices, int32_t* index, double* part_v, int32_t* part_i, int unfolded, hipStream_t stream);
hipError_t launch_llh_const(int64_t n_rep, const double* jsfs, double* consts, int unfolded, hipStream_t stream);
hipError_t launch_llk(int64_t n_cand, const double* jafs, const int32_t* status, int64_t n_rep, const double* jsfs,
                      const double* consts, double* llk, int unfolded, hipStream_t stream);
// llk[c] = the log-likelihood of candidate c against ITS OWN replicate row[c] (-inf where status[c] != MISTI_OK): the rows path of
// the batched search (misti_nm_solve_rows).  Same expressions as the inline epilogue and llk_kernel: the same bits.
hipError_t launch_llk_rows(int64_t n, const double* jafs, const int32_t* status, const int32_t* row, const double* jsfs,
                           const double* consts, double* llk, int unfolded, hipStream_t stream);

// Curvature at a point (misti_curvature, misti_curvature_assemble_dev): a point of D parameters has M = 1 + 2 D^2 stencil candidates.
// launch_curv_stencil: h[P][D] and point_status[P] (MISTI_CURV_BOUNDARY or 0), slot[P] (the point's rank among the points that have a
// stencil, -1 without: an exclusive scan on the device), and the candidates of those points in compacted arrays c_* ([cap * M] rows;
// c_bounds / c_pulses with nb2 / np integers per row, NULL with 0); `cap` is the host's own count of such points and bounds every write.
hipError_t launch_curv_stencil(int64_t n_point, int D, const double* x, const double* split, const int32_t* bounds, int nb2,
                               const int32_t* pulses, int np, double rel_step, double abs_step, int64_t cap, double* h, int32_t* point_status,
                               int32_t* slot, double* c_split, double* c_params, int32_t* c_bounds, int32_t* c_pulses, hipStream_t stream);
// dlog[P][D][7] / d2log[P][D][D][7] (either may be NULL) and point_status[P] from the stencil's spectra jafs[.][M][7] and statuses
// (NULL: all OK); point p's spectra start at row slot[p] * M (slot NULL: p * M), a point with slot[p] < 0 keeps pre_status[p].
hipError_t launch_curv_assemble(int64_t n_point, int D, int unfolded, const double* jafs, const int32_t* status, const double* h,
                                const int32_t* slot, const int32_t* pre_status, double* dlog, double* d2log, int32_t* point_status,
                                hipStream_t stream);
// grad[P][D] / hess[P][D][D]: dlog / d2log contracted with the class counts of row[p]; with llh0 (then jafs, slot and consts are
// needed too) the log-likelihood of every point's centre against its row, llk_rows_kernel's bits.
hipError_t launch_curv_contract(int64_t n_point, int D, int unfolded, const double* dlog, const double* d2log, const int32_t* point_status,
                                const int32_t* row, const double* jsfs, double* grad, double* hess, const double* jafs, const int32_t* slot,
                                const double* consts, double* llh0, hipStream_t stream);

}  // namespace misti
