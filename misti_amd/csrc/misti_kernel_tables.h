// The __constant__ tables and the method constants of the chain / trunk / spectrum path.  Defined here, so this header belongs to ONE
// translation unit, misti_kernels.hip (the build is -fno-gpu-rdc: a second one would get tables of its own that nobody uploads);
// upload_tables() there fills them.  Read by the pair chain (c_inv), the two-population interval and the candidate kernel.
#pragma once
#include "misti_device.h"

namespace misti {

__constant__ DevTables c_tab;
__constant__ double c_inv[INV_TABLE];   // c_inv[k] = 1/k: series terms divide by k (an fp64 division costs ~40 instructions)
// Terms of the uniformisation series as a function of q = (largest exit rate) x (interval length): the series stops after term K,
// the first k with e^-q q^(k-1) / (k-1)! < 1e-19 and k > q.  c_qmax[K] = the largest q for which K terms suffice (increasing in K;
// c_qmax[1] < 0: never one term), so K(q) = 1 + #{ j >= 1 : c_qmax[j] < q } - a compare, a ballot and a population count per 64
// entries instead of a running bound, a conversion and two compares inside every term (twopop_interval).
constexpr int QMAX_TABLE = 320;         // Q_SWITCH = 96 needs K <= 240
__constant__ double c_qmax[QMAX_TABLE];

// exp(M T) P0 and the occupation integral per interval, two methods:
//  * q = (largest exit rate) x (interval length) <= Q_SWITCH: uniformisation series
//    (cost ~ q + 8 sqrt(q) + 10 sparse mat-vecs, all terms non-negative);
//  * q > Q_SWITCH (a runaway corrected rate; the reference's dense Pade expm handles it by
//    squaring): Talbot contour quadrature  exp(A) v = sum_k -c_k (z_k - A)^-1 v  on the
//    "modified Talbot" cotangent contour of Trefethen, Weideman & Schmelzer (BIT 46, 2006),
//    N = 28 nodes (14 conjugate pairs; truncation 3.89^-N, measured error < 1e-15 here),
//    each shifted system solved by Jacobi sweeps with the same sparse row gather (the
//    coalescence part of the generator is nilpotent, so the sweeps terminate in <= 7 steps
//    unless migration is strong in both directions).  Cost is independent of q.  Where the sweeps
//    diverge or do not settle (two-way migration, mu T >~ 8) the series takes the interval in
//    ceil(q / Q_SWITCH) sub-steps, up to SUBSTEP_MAX (MISTI_STIFF beyond).
constexpr double Q_SWITCH = 96.0;
constexpr int JACOBI_MAX = 600;
constexpr int JACOBI_WATCH = 32;     // sweeps before the wave-wide stop and divergence tests start
constexpr int JACOBI_FLOOR = 48;     // sweeps from which a change within 1e-14 of the largest component is converged
constexpr double JACOBI_BLOWUP = 1e12;   // an iterate this large: the sweeps diverge
constexpr int SUBSTEP_MAX = 256;     // series sub-steps where the contour solve fails: q up to 256 Q_SWITCH, MISTI_STIFF beyond
constexpr long long FOLLOW_SPIN_LIMIT = 1LL << 22;   // polls (~1 us each) before a following trunk wave gives up

}  // namespace misti
