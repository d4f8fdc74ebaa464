// The chain state machine: correct_body, the lambda correction of one chain (or of one candidate's tail) as a resumable loop of
// residual batches and trust-region bookkeeping, with its cycle stamps and statistics, and wrong_phase.
// Instantiated by correct_kernel, correct_resume_kernel, correct_follow_kernel and post_kernel behind every batch entry; held by
// tests/test_gpu_golden.py, test_gpu_solver_trace.py, test_gpu_campaign.py and the parity lists of tests/parity.py.
#pragma once
#include <stdint.h>

#include "misti_device.h"
#include "misti_lsq.h"
#include "misti_model.h"
#include "misti_pair.h"
#include "misti_wave.h"

namespace misti {

// ------------------------------------------------ two-population correction --
// MigrationInference.CorrectLambdas, loop t < splitT (:311-354).  All values are
// wave-uniform except inside pair_eval.  Returns false on "correction failed".

// A packed launch whose long chains YIELD to the resume launch finishes most chains itself (BASELINE config 3: 91 %).  What waits for a
// chain - its trunk, the tails and the candidate kernel of its members - therefore runs in two PHASES: phase 1 (the chains the packed
// launch completed) on a second stream BESIDE the resume launch, phase 2 (the chains that yielded) behind it; phase 0 = no split (every
// other launch shape).  resume_t[ch] is -1 for a completed chain, the interval it resumes at otherwise.
__device__ __forceinline__ bool wrong_phase(const ChainBufs& cb, int64_t ch, int phase) {
    return phase != 0 && ((cb.resume_t[ch] >= 0) != (phase == 2));
}

// Kernel 1: lambda correction of the two-population intervals (CorrectLambdas loop t < splitT,
// MigrationInference.py:307-354; SolveLambdaSystem, CorrectLambda.py:266-317).
//
// The recursion over intervals does not depend on the split time except for where it stops:
// candidates with the same parameter vector share one CHAIN (discover_kernel), computed
// once up to the largest split index of its members - in a split x rate sweep 64 chains instead of
// 4 096.  A fractional split shortens the candidate's last two-population interval; that one
// interval is a TAIL, run per candidate from the chain's state (TAIL = true, in post_kernel).
//
// GROUP lanes per work item (64, 32, 16, 8 or 6; six carry the residual evaluations), no LDS beyond the staged grid.
// Each item runs its own resumable state machine: one pass of the loop = one residual batch
// (trial point + its forward-difference points) + the trust-region bookkeeping of
// trf_no_bounds (trf.py:401-560), so the items of a wavefront never wait for each other
// interval by interval.
template <bool CPFIT, int GROUP, bool TAIL, bool PRE = false>
__device__ __forceinline__
void correct_body(const DevModel& m, int64_t n_items, const ChainBufs& cb, const double* __restrict__ split_time, const double* __restrict__ params,
                  int64_t block, double* lds, double* lc_sh = nullptr, volatile int* flags = nullptr, double* pre = nullptr,
                  const int32_t* chain_map = nullptr, int yield_nfev = 0, int t_start = 0, int phase = 0) {
    const int lane = lane_id();
    const int sub = lane % GROUP;
    const int64_t n_live = TAIL ? n_items : (int64_t)cb.n_chains[0];
    // GROUP = 6 packs ten items into a wave; its last four lanes belong to no item
    const int64_t pos = (lane / GROUP < 64 / GROUP) ? (block * (64 / GROUP)) + (lane / GROUP) : n_live;
    if (TAIL) {
        // a wave none of whose items has a fractional split has nothing to do: leave before staging
        bool mine = false;
        if (pos < n_live) { const double st = split_time[pos]; mine = st != floor(st); }
        if (!__any(mine)) {
            if (pos < n_live && sub == 0) cb.tail_status[pos] = MISTI_OK;
            return;
        }
    } else if (block * (64 / GROUP) >= n_live) return;
    // chains of a packed launch (chain_map): position -> chain by descending length, so that the longest start first and the
    // chains sharing a wave are of similar length; a chain's bits do not depend on where it runs
    const int64_t slot = (!TAIL && chain_map && pos < n_live) ? (int64_t)chain_map[pos] : pos;
    // the shared grid (interval lengths, PSMC rates) staged in LDS: every pass of the state
    // machine of some item reads it, and an L2 round trip per read dominated the kernel
    {
        const int nt = m.numT - 1, nl = 2 * m.numT;
        for (int i = lane; i < nt; i += 64) lds[i] = m.times[i];
        for (int i = lane; i < nl; i += 64) lds[nt + i] = m.lh[i];
    }
    lds_fence();                                   // staged and read by this wavefront only
    if (pos >= n_live) return;
    const int64_t cand = TAIL ? slot : (int64_t)cb.rep[slot];      // whose parameters (chains: slot IS the chain id, see correct_kernel)
    const double* par = params ? params + cand * m.n_param : nullptr;
    Grid G;
    int status;
    int t = 0;
    double* lc_w;     // lc_w[2 t + k]        corrected rates of interval t
    double* tr_w;     // tr_w[6 (t + 1) + j]  pair state after interval t
    PairState ps;
    const int32_t* bb = cb.bounds ? cb.bounds + cand * 2 * m.n_band : nullptr;
    const int32_t* pt = cb.pulse_times ? cb.pulse_times + cand * m.n_pulse : nullptr;
    int32_t* sv_w = nullptr;   // sv_w[t]  solver word of interval t (trace on)
    double* it_w = nullptr;    // it_w[(t * MISTI_TRACE_MAX_ITER + i) * 2 + k]  trial points of the unbounded solve of interval t
    if (!TAIL) {
        status = MISTI_OK;
        for (int i = 0; i < m.n_param; ++i) if (par[i] < 0) status = MISTI_NEG_PARAM;
        G.numT0 = m.numT; G.numT = m.numT; G.split = chain_len(cb, slot); G.ins = -1; G.frac = 0.0;
        if (cb.solver) sv_w = cb.solver + slot * (int64_t)m.numT;
        if (cb.iters && slot < cb.iter_cap) it_w = cb.iters + slot * (int64_t)m.numT * MISTI_TRACE_MAX_ITER * 2;
        lc_w = cb.lc + slot * (int64_t)m.numT * 2;
        tr_w = cb.trace + slot * (int64_t)(m.numT + 1) * 6;
        ps.p[0][0] = 1; ps.p[0][1] = 0; ps.p[0][2] = 0;
        ps.p[1][0] = 0; ps.p[1][1] = 1; ps.p[1][2] = 0;
        if (t_start > 0) {
            // a chain that YIELDED in the packed launch (see below) resumes at the interval it was in: the pair state before
            // interval t_start is in its trace, and a solve restarted from the same state is the same solve
            t = t_start;
            const double* r = tr_w + 6 * t_start;
            ps.p[0][0] = r[0]; ps.p[1][0] = r[1]; ps.p[0][1] = r[2]; ps.p[1][1] = r[3]; ps.p[0][2] = r[4]; ps.p[1][2] = r[5];
        } else if (sub == 0) { tr_w[0] = 1; tr_w[1] = 0; tr_w[2] = 0; tr_w[3] = 1; tr_w[4] = 0; tr_w[5] = 0; }
    } else {
        status = setup_candidate(m, split_time[cand], par, G, bb, pt);
        if (sub == 0) cb.tail_status[cand] = MISTI_OK;
        if (status != MISTI_OK || G.ins < 0) return;               // nothing to do: no fractional split
        if (cb.tail_solver) sv_w = cb.tail_solver + cand - G.ins;
        const int64_t ch = chain_of(cb, cand);
        if (wrong_phase(cb, ch, phase)) return;                    // this chain's members belong to the other phase's launch
        if (cb.fail_t[ch] < G.ins) return;                         // the chain failed before this candidate's tail
        t = G.ins;
        const double* r = cb.trace + (ch * (int64_t)(m.numT + 1) + t) * 6;
        ps.p[0][0] = r[0]; ps.p[1][0] = r[1]; ps.p[0][1] = r[2]; ps.p[1][1] = r[3]; ps.p[0][2] = r[4]; ps.p[1][2] = r[5];
        lc_w = cb.tail_lc + 2 * cand - 2 * (int64_t)t;
        tr_w = cb.tail_state + 6 * cand - 6 * (int64_t)(t + 1);
    }
    G.times = lds; G.lh = lds + (m.numT - 1);
    Model mod{&m, par, G.split, {0, 0, 0, 0}};
    mod.bb = bb;
    mod.pt = pt;
    mod.cache();
    const bool correct = !(m.flags & MISTI_TRUE_EPS);
    const int max_nfev = 200;                    // 100 * n (least_squares.py)
    Diag dg;
#ifdef MISTI_TREE_STATS
    int ts_tree = 0, ts_miss = 0, ts_cons = 0, ts_miss_at[6] = {0, 0, 0, 0, 0, 0};
#endif

    // solver state of the interval in progress
    PairProblem pb;
    double x[2] = {0, 0}, f[2] = {0, 0}, J[2][2] = {{0, 0}, {0, 0}}, g[2] = {0, 0}, xe[2] = {0, 0}, p[2] = {0, 0}, vk[3] = {0, 0, 0};
    double cost = 0.0, Delta = 0.0, alpha = 0.0, predicted = 0.0;
    int nfev = 0;
    bool first = false, in_solve = false;
    bool yielded = false;      // packed launch: this chain left at interval t for correct_resume_kernel
    bool noise_go = false;     // default fit: the solve went on past a gradient test its noise-free residual satisfied (ect_noise_continues)
    bool stalled = false;      // default fit: the stall rule returned the starting point (trace bit MISTI_TRACE_STALL_BIT; nfev stays what was evaluated)
    // speculative slots (one chain per wave only): SPEC_SLOTS x 6 lanes, slot 0 = the point the solver asked for
    constexpr bool SPEC = (GROUP == 64) && !TAIL;
    constexpr int SPEC_SLOTS = 10;
    const int slot_of_lane = SPEC ? (lane < 6 * SPEC_SLOTS ? lane / 6 : 0) : 0;
    const int role = SPEC ? (lane < 6 * SPEC_SLOTS ? lane % 6 : (lane - 6 * SPEC_SLOTS) % 6) : sub;   // lanes beyond the slots repeat slot 0
    int spec_axis = -1;        // >= 0: the solver is in the exact rank-one regime and moves along this axis
    int vk_base = 0;           // first lane of the slot whose state vectors vk belong to the accepted point

    auto finish_interval = [&](double lc0, double lc1, int32_t word) -> bool {       // :345-350; false = correction failed
        if (sub == 0) { lc_w[2 * t] = lc0; lc_w[2 * t + 1] = lc1; if (sv_w) sv_w[t] = word; }
        if (uni<GROUP>(!(lc0 > 0) || !(lc1 > 0))) {
            status = (isnan(lc0) || isnan(lc1)) ? MISTI_NUMERIC : MISTI_CORR_FAILED;
            return false;
        }
        if (sub == 0) {
            double* r = tr_w + 6 * (t + 1);
            r[0] = ps.p[0][0]; r[1] = ps.p[1][0]; r[2] = ps.p[0][1]; r[3] = ps.p[1][1]; r[4] = ps.p[0][2]; r[5] = ps.p[1][2];
        }
        if (!TAIL && lc_sh) {
            // hand the interval to the trunk wave of this workgroup (correct_follow_kernel): rates, then the count
            if (sub == 0) { lc_sh[2 * t] = lc0; lc_sh[2 * t + 1] = lc1; }
            lds_order();
            if (sub == 0) lds_put(flags, t + 1);
        }
        ++t;
        return true;
    };

#ifdef MISTI_STAMP
    long long c_adv = 0, c_batch = 0, c_book = 0, c_t0 = 0, c_collect = 0, c_update = 0, c_next = 0, c_tree = 0;
#define STAMP(acc) { long long now_ = clock64(); acc += now_ - c_t0; c_t0 = now_; }
#else
#define STAMP(acc)
#endif
    bool active = status == MISTI_OK;
    if (PRE) {
        // What an interval needs that does not depend on the recursion - migration rates, pulse, exp(-lh T) of both
        // genomes - for all intervals at once, one interval per lane, instead of a band-table walk and two exponentials on
        // the critical path of every interval.  Same expressions as below, so the same bits.
        if (active)
            for (int tt = lane; tt < G.split; tt += 64) {
                double a0, a1, b0, b1;
                mod.mig(tt, a0, a1);
                mod.pulse(tt, b0, b1);
                const double Tt = G.T(tt);
                double* q = pre + 6 * tt;
                q[0] = a0; q[1] = a1; q[2] = b0; q[3] = b1; q[4] = exp(-G.lhk(tt, 0) * Tt); q[5] = exp(-G.lhk(tt, 1) * Tt);
            }
        lds_fence();
    }
#ifdef MISTI_STAMP
    c_t0 = clock64();
#endif
    while (uni<GROUP>(active)) {
        if (uni<GROUP>(!in_solve)) {
            // ---- advance over intervals until one needs the iterative solver ----------
            while (uni<GROUP>(t < G.split)) {
                double pu0, pu1, mu0, mu1, eh0 = 0.0, eh1 = 0.0;
                if (PRE) { const double* q = pre + 6 * t; mu0 = q[0]; mu1 = q[1]; pu0 = q[2]; pu1 = q[3]; eh0 = q[4]; eh1 = q[5]; }
                else { mod.pulse(t, pu0, pu1); mod.mig(t, mu0, mu1); }
                pulse_pairs<GROUP>(ps, pu0, pu1);                                       // :315-323
                double lh0 = G.lhk(t, 0), lh1 = G.lhk(t, 1);
                if (!correct) { if (uni<GROUP>(!finish_interval(lh0, lh1, 0))) break; continue; }    // :325-326
                const double T = G.T(t);
                const double s0 = (ps.p[0][0] + ps.p[0][1]) + ps.p[0][2];
                const double s1 = (ps.p[1][0] + ps.p[1][1]) + ps.p[1][2];
                if (m.mixture_th > 0.0) {                                               // CorrectLambda.py:267-272 (threshold 0 never fires)
                    double mix = 0.0;
                    for (int i = 0; i < 3; ++i) { double d = ps.p[0][i] / s0 - ps.p[1][i] / s1; mix += d * d; }
                    if (sqrt(mix) < m.mixture_th) { finish_interval(-1.0, -1.0, 0); break; }
                }
                if (uni<GROUP>(mu0 + mu1 < 1e-10)) {
                    double lc0, lc1;
                    int32_t word = solver_word(0, 0, 1);
                    if (CPFIT) {
                        // SolveNoMigration1 :213-235
                        double A1 = ps.p[0][0] / s0, A2 = ps.p[0][1] / s0, A3 = ps.p[1][0] / s1, A4 = ps.p[1][1] / s1;
                        double C1 = ps.p[0][2] / s0, C2 = ps.p[1][2] / s1;
                        double D = A1 * A4 - A2 * A3;
                        double B1 = A4 / D, B2 = -A2 / D, B3 = -A3 / D, B4 = A1 / D;
                        if (!PRE) { eh0 = exp(-lh0 * T); eh1 = exp(-lh1 * T); }
                        double X1 = eh0 - C1, X2 = eh1 - C2;
                        double y0 = B1 * X1 + B2 * X2, y1 = B3 * X1 + B4 * X2;
                        if (uni<GROUP>(y0 > 0 && y1 > 0)) { lc0 = -log(y0) / T; lc1 = -log(y1) / T; }
                        else { lc0 = lc1 = -1.0; }
                    } else {
                        // SolveNoMigration :253-264: bounded 2-D fit of the conditional expected coalescence time
                        double pr[2][3];
                        for (int i = 0; i < 3; ++i) { pr[0][i] = ps.p[0][i] / s0; pr[1][i] = ps.p[1][i] / s1; }
                        double tgt0 = ect_one_pop(lh0, T), tgt1 = ect_one_pop(lh1, T);
                        auto resid = [&](const double l[2], double ff[2]) {          // LambdaSystemNoMigration :237-251
                            double e0 = exp(-l[0] * T), e1 = exp(-l[1] * T);
                            double n0 = ect_noncond(l[0], T), n1 = ect_noncond(l[1], T);
                            for (int k = 0; k < 2; ++k) {
                                double pnc = pr[k][0] * e0 + pr[k][1] * e1 + pr[k][2];
                                double ct = (pr[k][0] * n0 + pr[k][1] * n1) / (1.0 - pnc);
                                ff[k] = ct - (k ? tgt1 : tgt0);
                            }
                        };
                        double xx[2] = {lh0, lh1};
                        word = trf_bounded<2>(resid, xx, 0.01 * fmin(lh0, lh1));
                        lc0 = xx[0]; lc1 = xx[1];
                    }
                    double e0 = exp(-lc0 * T), e1 = exp(-lc1 * T);
                    for (int k = 0; k < 2; ++k) { ps.p[k][0] *= e0; ps.p[k][1] *= e1; }
                    if (uni<GROUP>(!finish_interval(lc0, lc1, word))) break;
                    continue;
                }
                // migrating interval: set the 2x2 problem up (:278-305) and leave the advance loop
                double n0 = 0, n1 = 0, nd = 0;
                for (int i = 0; i < 3; ++i) { n0 += ps.p[0][i] * ps.p[0][i]; n1 += ps.p[1][i] * ps.p[1][i]; double d = ps.p[0][i] - ps.p[1][i]; nd += d * d; }
                bool averaged = false;
                if (uni<GROUP>(nd < 0.0004 * fmin(n0, n1))) { double mean = (lh0 + lh1) / 2.0; lh0 = lh1 = mean; averaged = true; }   // normD < 0.02 min(norms), squared
                pb.mu0 = mu0 * T; pb.mu1 = mu1 * T;                                      // stretch :293-298
                const double lhs0 = lh0 * T, lhs1 = lh1 * T;
                const bool g1 = role & 1;                                                // this lane's genome
                for (int i = 0; i < 3; ++i) pb.Pk[i] = g1 ? ps.p[1][i] : ps.p[0][i];
                pb.sk = g1 ? s1 : s0;
                // "empty": below 1e-30 of the genome's total - what one interval with rate x length > 70 leaves; far below
                // the rounding of every sum the state enters (it is dropped, not carried)
                pb.red = !CPFIT ? 0 : (pb.mu1 == 0.0 && ps.p[0][0] <= PAIR_EMPTY * s0 && ps.p[1][0] <= PAIR_EMPTY * s1) ? 1
                                    : (pb.mu0 == 0.0 && ps.p[0][1] <= PAIR_EMPTY * s0 && ps.p[1][1] <= PAIR_EMPTY * s1) ? 2 : 0;
                if (uni<GROUP>(!PRE || averaged)) { eh0 = exp(-lhs0); eh1 = exp(-lhs1); }
                if (CPFIT) { const double t0_ = eh0 * s0, t1_ = eh1 * s1; pb.tgtk = g1 ? t1_ : t0_; }
                else {
                    double pa = eh0, pbb = eh1;                                          // ExpectedCoalTimeOnePopTmp, T = 1
                    const double t0_ = 1.0 / lhs0 - 1.0 / (1.0 / pa - 1.0);
                    const double t1_ = 1.0 / lhs1 - 1.0 / (1.0 / pbb - 1.0);
                    pb.tgtk = g1 ? t1_ : t0_;
                }
                xe[0] = lhs0; xe[1] = lhs1;
                first = true; in_solve = true; spec_axis = -1;
                break;
            }
            if (uni<GROUP>(!in_solve)) { active = false; break; }  // reached the split, or failed
        }
        STAMP(c_adv)
        // ---- yield (packed launches only) ----------------------------------------------------------------------------------
        // A solve that has not converged after yield_nfev evaluations is a rate running away: tens to hundreds of evaluations,
        // interval after interval, each of them alone in its six lanes - a packed launch ends with its few such chains (16 384
        // random starts: 9 % of the chains, 3 x the mean evaluation count; the average wave lives a third of the kernel).  The chain
        // leaves here and is RESUMED at this interval, one chain per wave with the speculation tree, by correct_resume_kernel.
        if (!TAIL && yield_nfev > 0 && in_solve && !first && nfev >= yield_nfev) { yielded = true; active = false; break; }
        // ---- one residual batch: the point the solver needs in slot 0, guesses of its successors in the other slots ----
        // One chain per wave leaves 58 of 64 lanes idle during an evaluation.  In the exact rank-one regime (a rate
        // decoupled after a runaway: its Jacobian column is exactly zero and the solver moves along the other axis by
        // +-Delta, see next_step) the iteration is a walk on a line whose next points are computable before the trial's
        // residual is known: the trial is accepted and the radius doubled (next point xe +- 2 Delta) or it is rejected
        // and the radius quartered (next point x + sign Delta/4) - 98 % of the steps of the reference's traces
        // (tests/golden/golden_traces.json.gz) - and the same again one level down.  The tree of those successors
        //        slot 0  the trial                     1, 2  0 accepted, doubled, then + / -        3  0 rejected
        //        4, 5    1 / 2 rejected                6, 7  3 accepted, doubled, then + / -        8  3 rejected
        //        9       6 rejected (the likeliest third step: rejected, accepted +, rejected)
        // is evaluated in the idle lanes (slot s = lanes 6 s .. 6 s + 5) by the same pure function of the point, and the
        // bookkeeping of all of them is then done at once, one hypothesis per slot (tree consume below): up to four
        // solver steps per pass, bit for bit the same iteration.  A guess never consumed costs nothing.
        double px0 = xe[0], px1 = xe[1];
        const bool tree = SPEC && uni<GROUP>(spec_axis >= 0 && !first);       // wave-uniform
        double Dpre_l = Delta, ps_l = 0.0;                                    // per slot: radius and signed step of its hypothesis
        if (tree) {
            const int k = __builtin_amdgcn_readfirstlane(spec_axis);
            const double pk = k == 0 ? p[0] : p[1];
            const bool pos = pk > 0;
            const double D2 = 2.0 * Delta;
            const double dq0 = 0.25 * sqrt64(p[0] * p[0] + p[1] * p[1]);      // radius after rejecting the trial (tr_update)
            const double dq1 = 0.25 * sqrt64(D2 * D2);                        // ... after accepting it, doubling, and rejecting that
            const double dq3 = 0.25 * sqrt64(dq0 * dq0);                      // ... after rejecting twice
            const double xk = k == 0 ? x[0] : x[1], xek = k == 0 ? xe[0] : xe[1];
            const double u = xk + (pos ? dq0 : -dq0);                         // slot 3's point
            const int sl = slot_of_lane;
            const double dq0x2 = 2.0 * dq0;
            const double dq6 = 0.25 * sqrt64(dq0x2 * dq0x2);                  // ... after rejecting, accepting the retry, doubling, rejecting
            const bool root = sl == 0 || sl == 3 || sl == 8;                  // hypotheses that keep the current point x
            Dpre_l = sl == 0 ? Delta : sl <= 2 ? D2 : sl == 3 ? dq0 : sl <= 5 ? dq1 : sl <= 7 ? dq0x2 : sl == 8 ? dq3 : dq6;
            const bool pos_l = root ? pos : (sl == 1 || sl == 4 || sl == 6 || sl == 9);
            ps_l = sl == 0 ? pk : (pos_l ? Dpre_l : -Dpre_l);
            const double from = root ? xk : (sl == 6 || sl == 7 || sl == 9) ? u : xek;
            const double at = from + ps_l;
            if (sl >= 1 && sl <= 9) { px0 = k == 0 ? at : xe[0]; px1 = k == 1 ? at : xe[1]; }
        }
        double res, w[3];
        bool guard_l = false;
        pair_eval<CPFIT>(pb, px0, px1, role, dg, res, w, guard_l);
        dg.evals += 1;
        STAMP(c_batch)
        int slot = 0;
        bool stop = false;
        bool look = false;
        if (tree) {
            // ---- tree consume: the bookkeeping of every slot under its own hypothesis, all slots at once ------------
            const int k = __builtin_amdgcn_readfirstlane(spec_axis);
            const int sl = slot_of_lane;
            double fnl[2], Jnl[2][2];
            bool finl;
            slot_collect(res, px0, px1, 6 * sl, fnl, Jnl, finl);
            const double cnl = 0.5 * (fnl[0] * fnl[0] + fnl[1] * fnl[1]);
            // the state a hypothesis starts from: the current one (slots 0, 3, 8), the trial accepted (1, 2, 4, 5: slot 0's
            // evaluation) or the retry accepted (6, 7: slot 3's evaluation).  One gather per quantity: lane 60 (idle, it
            // repeats slot 0) is lent the current state, so every slot pulls from lane 60, 0 or 18.
            double xp[2], fp[2], Jp[2][2], cp;
            {
                const bool lend = lane == 60;
                const int src = (sl == 1 || sl == 2 || sl == 4 || sl == 5) ? 0 : (sl == 6 || sl == 7 || sl == 9) ? 18 : 60;
                fp[0] = __shfl(lend ? f[0] : fnl[0], src, 64); fp[1] = __shfl(lend ? f[1] : fnl[1], src, 64);
                for (int r = 0; r < 2; ++r) for (int c = 0; c < 2; ++c) Jp[r][c] = __shfl(lend ? J[r][c] : Jnl[r][c], src, 64);
                cp = __shfl(lend ? cost : cnl, src, 64);
                xp[0] = __shfl(lend ? x[0] : px0, src, 64); xp[1] = __shfl(lend ? x[1] : px1, src, 64);
            }
            double gp[2], pl[2];
            gp[0] = Jp[0][0] * fp[0] + Jp[1][0] * fp[1];
            gp[1] = Jp[0][1] * fp[0] + Jp[1][1] * fp[1];
            pl[0] = k == 0 ? ps_l : 0.0; pl[1] = k == 1 ? ps_l : 0.0;
            const double predl = predicted_of(Jp, pl, gp);
            double Dl = Dpre_l, dql;
            int terml;
            bool accl;
            tr_update(finl, pl, xp, cp, cnl, predl, Dl, dql, terml, accl);
            // the state after the step and what the solver does next (the tests of the serial loop below and of next_step)
            double xs[2], fs[2], Js[2][2], gs[2];
            xs[0] = accl ? px0 : xp[0]; xs[1] = accl ? px1 : xp[1];
            fs[0] = accl ? fnl[0] : fp[0]; fs[1] = accl ? fnl[1] : fp[1];
            const double cs = accl ? cnl : cp;
            for (int r = 0; r < 2; ++r) for (int c = 0; c < 2; ++c) Js[r][c] = accl ? Jnl[r][c] : Jp[r][c];
            gs[0] = Js[0][0] * fs[0] + Js[1][0] * fs[1];
            gs[1] = Js[0][1] * fs[0] + Js[1][1] * fs[1];
            const double g_norm = fmax(fabs(gs[0]), fabs(gs[1]));
            const bool donel = terml != 0 || (accl && (g_norm < LSQ_GTOL || !(g_norm < INFINITY)));
            const bool z0 = Js[0][0] == 0.0 && Js[1][0] == 0.0, z1 = Js[0][1] == 0.0 && Js[1][1] == 0.0;
            const bool same_axis = (z0 != z1) && (z0 ? 1 : 0) == k;
            const bool plus = !((k == 0 ? gs[0] : gs[1]) > 0);                 // next_step: pk = gk > 0 ? -Delta : Delta
            // outcome: 1 / 2 accepted, radius doubled, next step + / -; 3 rejected, radius quartered, same direction again;
            // 0 anything else (termination, a kept radius, another regime): the serial loop below takes it from there
            int codel = 0;
            if (!donel && same_axis) {
                if (accl) codel = Dl == 2.0 * Dpre_l ? (plus ? 1 : 2) : 0;
                else codel = (Dl == dql && plus == (ps_l > 0)) ? 3 : 0;
            }
            // ---- walk the tree along the outcomes that came true (wave-uniform) ----
            int cur = 0, last = -1, last_acc = -1, consumed = 0;
            for (;;) {
                if (nfev + 1 >= max_nfev) break;                               // the budget test belongs to the serial loop
                const int at = 6 * cur;
                const int code = __builtin_amdgcn_readlane(codel, at);
                if (code == 0) break;
                if (it_w && sub == 0 && nfev < MISTI_TRACE_MAX_ITER) {
                    double* r = it_w + ((int64_t)t * MISTI_TRACE_MAX_ITER + nfev) * 2;
                    r[0] = bcast(px0, at); r[1] = bcast(px1, at);
                }
                ++nfev; ++consumed; last = cur;
                if (__builtin_amdgcn_readlane((int)guard_l, at)) dg.guard = true;
                if (__builtin_amdgcn_readlane((int)accl, at)) last_acc = cur;
                int child = -1;
                if (cur == 0) child = code;
                else if (cur == 1) child = code == 3 ? 4 : -1;
                else if (cur == 2) child = code == 3 ? 5 : -1;
                else if (cur == 3) child = code == 1 ? 6 : code == 2 ? 7 : 8;
                else if (cur == 6) child = code == 3 ? 9 : -1;
#ifdef MISTI_TREE_STATS
                if (child < 0) { ts_miss += 1; ts_miss_at[cur == 1 || cur == 2 ? 0 : cur == 4 || cur == 5 ? 1 : cur == 7 ? 2 : cur == 8 ? 3 : cur == 9 ? 4 : 5] += 1; }
#endif
                if (child < 0) break;
                cur = child;
            }
#ifdef MISTI_TREE_STATS
            ts_tree += 1; ts_cons += consumed;
#endif
            if (consumed > 0) {
                const int at = 6 * last;
                x[0] = bcast(xs[0], at); x[1] = bcast(xs[1], at);
                f[0] = bcast(fs[0], at); f[1] = bcast(fs[1], at);
                for (int r = 0; r < 2; ++r) for (int c = 0; c < 2; ++c) J[r][c] = bcast(Js[r][c], at);
                cost = bcast(cs, at);
                Delta = bcast(Dl, at);
                if (last_acc >= 0) { vk[0] = w[0]; vk[1] = w[1]; vk[2] = w[2]; vk_base = 6 * last_acc; }
                g[0] = J[0][0] * f[0] + J[1][0] * f[1];
                g[1] = J[0][1] * f[0] + J[1][1] * f[1];
                // the step after a consumed slot is again the rank-one one along k (that is what its outcome code says):
                // next_step's rank-one branch, without the rest of it
                const double pk = (k == 0 ? g[0] : g[1]) > 0 ? -Delta : Delta;
                p[0] = k == 0 ? pk : 0.0; p[1] = k == 1 ? pk : 0.0;
                alpha = 0.0;
                predicted = predicted_of(J, p, g);
                xe[0] = x[0] + p[0]; xe[1] = x[1] + p[1];
                dg.spec += consumed - 1;
                look = true;
            }
            STAMP(c_tree)
        }
        // ---- consume: trust-region bookkeeping (trf_no_bounds) for the needed point, and again while the next point
        //      asked for is one of those evaluated in this pass ---------------------------------------------------
        for (;; look = true) {
            if (look) {
                // was the point now needed evaluated in this pass?  (lanes of role 0 carry their slot's point)
                const unsigned long long hit = __ballot(role == 0 && lane < 6 * SPEC_SLOTS && px0 == xe[0] && px1 == xe[1]);
                if (hit == 0) break;
                slot = (__ffsll((long long)hit) - 1) / 6;
                dg.spec += 1;
            }
            double fn[2], Jn[2][2];
            bool finite;
            if (it_w && sub == 0) {
                const int i = first ? 0 : nfev;
                if (i < MISTI_TRACE_MAX_ITER) { double* r = it_w + ((int64_t)t * MISTI_TRACE_MAX_ITER + i) * 2; r[0] = xe[0]; r[1] = xe[1]; }
            }
            const int base = SPEC ? 6 * slot : 0;
            pair_collect<GROUP>(res, xe, base, fn, Jn, finite);
            STAMP(c_collect)
            if (SPEC) { if (__builtin_amdgcn_readlane((int)guard_l, __builtin_amdgcn_readfirstlane(base))) dg.guard = true; }
            else if (guard_l) dg.guard = true;
            bool accept = false, done = false;
            int term = 0;
            double cost_new = 0.5 * (fn[0] * fn[0] + fn[1] * fn[1]);
            if (uni<GROUP>(first)) {
                first = false;
                nfev = 1;
                if (uni<GROUP>(!finite)) { status = MISTI_NUMERIC; active = false; stop = true; break; }   // SciPy raises on a non-finite start
                Delta = sqrt64(xe[0] * xe[0] + xe[1] * xe[1]);
                if (Delta == 0) Delta = 1.0;
                alpha = 0.0;
                accept = true;
#ifndef MISTI_NO_STALL_RULE
                if (!CPFIT) {
                    // ---- default fit: would the REFERENCE's solve get anywhere from here? ---------------------------------------------
                    // Its residual T M^-1 e^{MT} p - M^-2 (e^{MT} - I) p carries ~eps / |M T|^2 of rounding noise (see ect_noise_continues); on a
                    // very short interval (rate x length ~1e-4: two nearly coincident time points of the merged grid) that noise, divided by the
                    // forward-difference step h = 1.5e-8, is LARGER than the Jacobian itself.  SciPy's iteration then takes steps a tenth of the
                    // needed size in random directions, rejects most of them, quarters its radius until xtol fires (status 3 after 14 - 23
                    // evaluations) and returns a point within ~0.3 % of where it started - 4 - 10 % from the root the noise-free series finds in
                    // three evaluations.  In the reference's own traces (tests/golden/*_traces.json.gz: 16 200 two-population default-fit solves
                    // of BASELINE's grids and the held-out grid config2b) EVERY one of the 205 solves with 0.29 W / h >= 2 |J| ended that way, and
                    // none of the 15 000 with 0.29 W / h <= 0.04 |J| (in between: 10 % of 239 at 0.15).  The starting point is what the reference
                    // returns there, so it is what is returned here: status 3 (the reference's xtol), with the trace word saying so - bit
                    // MISTI_TRACE_STALL_BIT - and nfev = 1, the evaluations actually made (the reference's own count there is 14 - 23; a
                    // made-up 19 used to stand here: ADVICE r5).  Its model of W is the one of the
                    // noise rule below (eps / (0.7 x 2 min(d0, d1)^2), calibrated in round 3).
                    // (Tried: no stall where one Gauss-Newton step of the noise-free residual leaves the positive quadrant - the reference fails
                    // there on config 3's start 4908 in all of its runs - : config 3 under the default fit then has 41 instead of 40 status
                    // mismatches and 2 instead of 0 candidates outside in the first pass; not kept.)
                    const double dmin = fmin(2.0 * pb.mu0 + xe[0], 2.0 * pb.mu1 + xe[1]);
                    const double wm = (0.5 * LSQ_EPS / 0.7) / (dmin * dmin);
                    const double jmax = fmax(fmax(fabs(Jn[0][0]), fabs(Jn[0][1])), fmax(fabs(Jn[1][0]), fabs(Jn[1][1])));
                    const double hh = fmin(fabs(fd_step(xe[0])), fabs(fd_step(xe[1])));
                    if (dmin > 0.0 && 0.29 * wm > jmax * hh) { term = 3; stalled = true; }
                }
#endif
            } else {
                ++nfev;
                const double Delta_old = Delta;
                double dq;
                tr_update(finite, p, x, cost, cost_new, predicted, Delta, dq, term, accept);
                if (uni<GROUP>(finite && term == 0 && alpha != 0.0)) alpha *= Delta_old * rcp64(Delta);   // trf.py:515
            }
            // accepted: the trial becomes the current point (selects; g recomputed from whatever (J, f) is current)
            const double xo0 = x[0], xo1 = x[1];         // base point of the step p
            x[0] = accept ? xe[0] : x[0]; x[1] = accept ? xe[1] : x[1];
            f[0] = accept ? fn[0] : f[0]; f[1] = accept ? fn[1] : f[1];
            cost = accept ? cost_new : cost;
            for (int r = 0; r < 2; ++r) for (int c = 0; c < 2; ++c) J[r][c] = accept ? Jn[r][c] : J[r][c];
            vk[0] = accept ? w[0] : vk[0]; vk[1] = accept ? w[1] : vk[1]; vk[2] = accept ? w[2] : vk[2];
            vk_base = accept ? base : vk_base;           // the lanes whose state vectors belong to the accepted point
            g[0] = J[0][0] * f[0] + J[1][0] * f[1];
            g[1] = J[0][1] * f[0] + J[1][1] * f[1];
            STAMP(c_update)
            if (term != 0) done = true;
            else if (accept) {
                const double g_norm = fmax(fabs(g[0]), fabs(g[1]));
                bool g_stop = g_norm < LSQ_GTOL;
#ifndef MISTI_NO_NOISE_RULE           // diagnostic build switch: the solver exactly as SciPy's tests see the noise-free residual
                if (!CPFIT) {
                    // the gradient test as the reference's noisy residual would see it (ect_noise_continues): only after a real step
                    if (uni<GROUP>(g_stop && nfev > 1 && nfev < max_nfev)) {
                        // Measuring the noise costs two evaluations of both forms (behind every solve it made the default fit's chains
                        // half again as slow, and with several chains per wave each measurement runs with one chain's lanes).  The
                        // width follows eps / min(d0, d1)^2 - the 1 / |M|^2 lost digits - within a factor 10 either way on 97 % of 1 020
                        // sampled solves (median 0.7): where the test's outcome is the same at a tenth and at ten times that model, it is
                        // taken from the model; the measurement decides the band in between.
                        const double ph = fmax(fabs(p[0] / fd_step(xo0)), fabs(p[1] / fd_step(xo1)));
                        const double dmin = fmin(2.0 * pb.mu0 + xo0, 2.0 * pb.mu1 + xo1);
                        const double wm = (0.5 * LSQ_EPS / 0.7) / (dmin * dmin);
                        const double nb = 0.29 * wm * ph;
                        const double jf2 = (J[0][0] * J[0][0] + J[0][1] * J[0][1]) + (J[1][0] * J[1][0] + J[1][1] * J[1][1]);
                        const double g2 = g_norm * g_norm, t2 = LSQ_GTOL * LSQ_GTOL;
                        const bool surely_on = dmin > 0.0 && g2 + 0.01 * (jf2 > 0 ? fmin(fmin(J[0][0] * J[0][0] + J[1][0] * J[1][0], J[0][1] * J[0][1] + J[1][1] * J[1][1]), jf2) : 0.0) * nb * nb >= t2;
                        const bool maybe_on = !(dmin > 0.0) || g2 + 100.0 * jf2 * nb * nb >= t2;
                        if (uni<GROUP>(surely_on)) { g_stop = false; noise_go = true; }
                        else if (uni<GROUP>(maybe_on)) {
#if MISTI_NOISE_PROBE
                            g_stop = !ect_noise_continues<GROUP>(pb, xo0, xo1, p, J, g, role);
#else
                            g_stop = !(g2 + jf2 * nb * nb >= t2);        // diagnostic build: the model alone
#endif
                            if (!g_stop) noise_go = true;
                        }
                    }
                }
#endif
                if (g_stop || nfev >= max_nfev || !(g_norm < INFINITY)) done = true;
            } else if (nfev >= max_nfev) done = true;
            if (uni<GROUP>(done)) {
                dg.max_nfev = nfev > dg.max_nfev ? nfev : dg.max_nfev;
                for (int i = 0; i < 3; ++i) { ps.p[0][i] = gbcast<GROUP>(vk[i], vk_base + 0); ps.p[1][i] = gbcast<GROUP>(vk[i], vk_base + 1); }   // :313-317
                in_solve = false;
                // OptimizeResult.status: the termination test that fired, 1 = gtol, 0 = evaluation budget (trf.py:452-456,556-558)
                const int code = term != 0 ? term : ((accept && fmax(fabs(g[0]), fabs(g[1])) < LSQ_GTOL) ? 1 : 0);
                const int32_t went_on = (noise_go ? MISTI_TRACE_NOISE_BIT : 0) | (stalled ? MISTI_TRACE_STALL_BIT : 0);
                noise_go = false;
                stalled = false;
                const double T = G.T(t);               // re-read (LDS) rather than carried through the solver loop
                if (uni<GROUP>(!finish_interval(x[0] / T, x[1] / T, solver_word(nfev, code, 3) | went_on))) { active = false; stop = true; }   // :312, :346-348
                break;
            }
            predicted = next_step<GROUP>(J, f, g, Delta, alpha, p, dg.lm, spec_axis);
            xe[0] = x[0] + p[0]; xe[1] = x[1] + p[1];
            STAMP(c_next)
            if (!SPEC) break;
        }
        if (uni<GROUP>(stop)) break;
        STAMP(c_book)
    }
    if (dg.guard) { status = MISTI_NUMERIC; if (!TAIL) t = 0; yielded = false; }       // an overflowing iterate was cut off somewhere
    if (sub == 0) {
        if (!TAIL) {
            double* r = cb.work + slot * 6;
            if (yielded) {
                cb.resume_t[slot] = t;
                cb.resume_list[atomicAdd(&cb.n_chains[3], 1)] = (int32_t)slot;
            } else {
                if (yield_nfev > 0) cb.resume_t[slot] = -1;               // a packed launch that lets chains yield: this one is complete (see chain_phase)
                cb.fail_t[slot] = (status == MISTI_OK) ? 0x7fffffff : t;   // t = the interval that failed
                cb.fail_status[slot] = status;
            }
            if (t_start > 0) { dg.evals += (int)r[0]; dg.dense += (int)r[1]; dg.terms += (int)r[2]; dg.spec += (int)r[3]; dg.lm += (int)r[5];
                               dg.max_nfev = dg.max_nfev > (int)r[4] ? dg.max_nfev : (int)r[4]; }     // counters of the part before the yield
            r[0] = dg.evals; r[1] = dg.dense; r[2] = dg.terms; r[3] = dg.spec; r[4] = dg.max_nfev; r[5] = dg.lm;
#ifdef MISTI_TREE_STATS
            r[1] = ts_tree; r[2] = ts_miss; r[3] = ts_cons; r[4] = ts_miss_at[0] * 1e6 + ts_miss_at[1] * 1e3 + ts_miss_at[2]; r[5] = ts_miss_at[3] * 1e6 + ts_miss_at[4] * 1e3 + ts_miss_at[5];
#endif
#ifdef MISTI_STAMP
            r[0] = (double)c_tree; r[1] = (double)(c_collect + c_update); r[2] = (double)c_next;
            r[3] = (double)c_adv; r[4] = (double)c_batch; r[5] = (double)c_book;
#endif
        } else {
            cb.tail_status[cand] = status;
        }
    }
}

}  // namespace misti
