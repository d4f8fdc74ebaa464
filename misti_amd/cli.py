#!/usr/bin/env python3
"""Command line with the option surface of the reference's ``MiSTI.py``
(``/root/reference/MiSTI.py:43-260``) on top of the HIP engine.

    python -m misti_amd.cli g1.psmc g2.psmc data.sfs 64 -mi 1 4 64 0.2 1 --cpfit -uf

Same positional arguments and options (``-o -wd -tol -mth -mi -pu --sdate --hetloss
--discr -rd --funits -uf --nosmooth --trueEPS --cpfit -bs --debug``), same printed
result line (``bs_id = ... splitT = ... time = ... migration rates ... llh = ...``,
MiSTI.py:240 - what the ``test.bs`` scripts grep), ``-o`` written only for ``-bs 0``
(MiSTI.py:248-249).  ``--psmcMode 1`` (experimental PSMC re-estimation) is not offered.

Batched extension (no reference counterpart; replaces the bash loops of ``test.bs/*.sh``
and the GNU-parallel recipe of ``README.md:110-115``):

    --grid-st A B [STEP]      scan split times A..B (inclusive), bands ending at the
                              given split time follow each candidate's split
    --grid-mi K LO HI N       N log-spaced values for the K-th optimised parameter
    --all-bs                  evaluate every row of the JSFS file as a replicate
    --bootstrap N             the rows of the JSFS file are CHUNKS (column 0 a chunk's length): N block-bootstrap replicates of them are drawn on
                              the device (misti_bootstrap_rows_dev) and the 1 + N-row table - row 0 the sum of all chunks - replaces the rows
                              before any mode sees them; implies --all-bs.  The stream is this project's own (Philox4x64-10 keyed by
                              (--bs-seed K, replicate): replicate r is the same row whatever N, rank or device), NOT the reference's
                              generateJSFS_bs.py, which draws from Python's Mersenne Twister.  --bs-normalize: the reference's normalize=True;
                              --bootstrap-out FILE keeps the table as a #MiSTI_JSFS file (--all-bs on it repeats the run).  Not offered with -bs K
    --parametric N            for a JSFS file WITHOUT chunks (one row): stage 1 is the ordinary fit of the data row at the given split and
                              -mi/-pu initial values (what this line prints without grid options); stage 2 draws N replicates of the data's
                              number of sites (--sites M: of M sites) from the spectrum at that fit on the device
                              (misti_parametric_rows_dev; --bs-seed K) and the table [data; replicates] replaces the rows before any
                              mode sees them; implies --all-bs.  CAVEAT: the sites are drawn INDEPENDENTLY, real sites are linked - intervals
                              from these replicates are narrower than a block bootstrap's on the same genome; where the file has chunks
                              --bootstrap remains the confidence statement (--sites M may pass an effective number of sites).
                              --bootstrap-out FILE keeps the table (--all-bs on it repeats stage 2).  Not offered with --bootstrap,
                              --bs-normalize (there is nothing to normalise) or -bs K
    --jackknife M             with --fit-st or --grid-solve (M >= 1): the rows of the JSFS file are CHUNKS, as for --bootstrap; the delete-M block
                              jackknife's table - row 0 the sum of all chunks, then G = ceil(chunks / M) leave-out rows, row g the chunks
                              outside group g added in chunk order - is made on the device (misti_jackknife_rows_dev) and replaces the
                              rows; implies --all-bs.  Deterministic: no seed.  Behind the lines of row 0 the mode prints `jackknife:`
                              lines in place of the bootstrap t-interval: for the fitted split (--fit-st) and every rate the estimate,
                              the bias-corrected jackknife estimate, the bias, the standard error, the t-interval and the groups used
                              (optimize.jackknife_estimate: the weighted delete-m jackknife, weights from column 0 of the table).
                              --jackknife 0: the file already IS such a table (row 0 the data, rows 1.. the leave-out rows), nothing is
                              made; --jackknife-out FILE keeps the table of --jackknife M (--jackknife 0 --all-bs on it repeats the run).
                              Not offered with --bootstrap, --parametric, -bs K, --se, --sweep / --sweep-pu, or a mode that scans (plain
                              grid mode, --top, --polish, --profile: the arg-max over a grid does not move when one block is left out)
    --grid-solve              with --grid-st and/or --all-bs: for every (row, split) pair the reference's Solve from the
                              -mi/-pu initial values (the --grid-mi mesh points as starts: the best per pair), all pairs
                              in ONE batched search on the device; per pair the line MiSTI.py:240 prints (the test.bs
                              loops' order: row outer, split inner), then the 97.5 % t-interval of bs_conf_int.ipynb
    --fit-st                  with --grid-st A B [STEP] (the INITIAL splits) and optionally --all-bs: the split time fitted, not
                              scanned - for every row one Nelder-Mead search over (optimised parameters, split time) from every
                              (start, initial split) pair, all in ONE batched search (misti_nm_solve_split); per row the MiSTI.py:240
                              line of the best search with the fitted, fractional splitT, then (--all-bs) the t-interval of
                              bs_conf_int.ipynb over the fitted splits.  Needs no optimised -mi / -pu: a model without one is a
                              one-coordinate search.  Not offered with --sweep, --sweep-pu, --gpus N > 1 or --devices
    --hops N                  with --fit-st or --grid-solve (N >= 1): every search becomes the reference's GLOBAL search, Solve(globalOpt=True) -
                              scipy.optimize.basinhopping with N hops, T = 0.5 and SciPy's defaults for the Nelder-Mead minimiser
                              (xatol = fatol = 1e-4, 200 iterations and evaluations per coordinate) - all searches in ONE batched call
                              (misti_basinhopping_split / misti_basinhopping_rows); with --fit-st the hops move the split as well.
                              The lines are those of the mode without hops, each followed by its accepted hops and failed
                              minimisations, and one line states hops, step and seed.  -tol does not apply (the reference's global
                              search ignores it too: MigrationInference.py:723-725).  Not offered with --sweep, --sweep-pu,
                              --gpus N > 1 or --devices
    --hop-step S              with --hops (refused without): the initial step size of the random displacement (default 0.5; the split
                              in grid-index units)
    --hop-seed K              with --hops (refused without): search j of a row draws from numpy.random.default_rng([K, j]) (default 0)
    --de POP GENS             with --fit-st or --grid-solve (where --hops is): every search becomes a DIFFERENTIAL EVOLUTION of POP members
                              (4 ... 256) over at most GENS generations inside the box - one misti_de_search call over all rows, every
                              generation ONE dense engine batch, no inner minimisations.  The rule is this project's own, not SciPy's
                              (best1bin, dither, deferred selection; include/misti_hip.h states it).  Needs a finite --box for EVERY
                              searched coordinate (the split included under --fit-st) and refuses otherwise; member 0 of every
                              population is the -mi/-pu initial values (--grid-mi is not offered; under --fit-st the first split of
                              --grid-st).  The lines are those of the mode without it, and one line states members, generations, F,
                              CR and seed.  Not offered with --hops, --se, --sweep, --sweep-pu, --gpus N > 1 or --devices
    --de-seed K               with --de (refused without): every random number is numpy.random.Philox(key=[K, j]), j the search's index
                              within its row (default 0)
    --de-F LO HI              with --de: the dither range of the differential weight (default 0.5 1)
    --de-CR C                 with --de: the crossover probability (default 0.7)
    --de-polish               with --de: one boxed Nelder-Mead call (misti_nm_solve_box, -tol) from the DE results; a search keeps the better
    --mcmc W STEPS            after any fit of --fit-st or --grid-solve (local, --hops or --de): an ENSEMBLE MCMC of W walkers (even, 4 ... 256)
                              over STEPS steps per printed fit, inside the box - one misti_ensemble_sample call over all fits, every
                              half-step ONE dense engine batch.  The affine-invariant stretch move; the rule is this project's own
                              (include/misti_hip.h states it).  Samples llh / T under a uniform prior on the box: needs a finite --box for
                              EVERY coordinate (the split included under --fit-st).  The initial ensemble is drawn around each fit
                              (--mcmc-spread) - or, where --de W GENS ran with the same W, it is DE's final population.  Behind every fit line one `mcmc:` line per coordinate: mean, median, 2.5 % and 97.5 %
                              quantiles, the autocorrelation time of the ensemble mean and the acceptance fraction; `(short)` where
                              fewer than 50 autocorrelation times were kept.  Not offered with --se, --sweep, --sweep-pu, --gpus N > 1
                              or --devices
    --mcmc-burn B             with --mcmc: kept steps dropped before the summary (default: half of them)
    --mcmc-thin K             with --mcmc: keep every K-th step (default 1)
    --mcmc-seed K             with --mcmc: every random number is numpy.random.Philox(key=[K, j]), j the fit's index within its row (default 0)
    --mcmc-spread S           with --mcmc: the initial walkers are the fit + S x (box width) x uniform(-1, 1), clipped (default 1e-2)
    --mcmc-temp T|auto        with --mcmc: the temperature (default 1).  auto: trace(H^-1 J) / p from the curvature at the data row's fit and
                              the bootstrap rows' class counts - the magnitude adjustment of a composite likelihood; needs --all-bs
    --mcmc-out FILE.npz       with --mcmc: the chains, their llh, the acceptance counters and the final ensembles
    --mcmc-ladder L RATIO     with --mcmc: PARALLEL TEMPERING (misti_tempered_sample) - per fit a ladder of L ensembles (1 ... 64) at the temperatures
                              T0 RATIO^(l / (L - 1)), T0 the temperature of --mcmc-temp (auto included), RATIO finite and > 1; every rung starts from
                              the ensemble the cold rung starts from, neighbouring rungs trade walkers, all rungs ride in the same engine batches.
                              The `mcmc:` / `post:` lines are the cold rung's; behind them one `ladder:` line per fit: the temperatures, the swap
                              acceptance per pair, the mean llh per rung and logz, the trapezoid estimate of log Z(1 / T0) - log Z(1 / T_max) under
                              the normalised uniform prior on the box (the piece above T_max is not in it; for a composite likelihood it means
                              something only at the calibrated temperature, --mcmc-temp auto).  --mcmc-out gains ladder, swap_proposed,
                              swap_accepted, rung_llh and logz; its chain is the cold rung's, its chain_llh every rung's
    --mcmc-swap E             with --mcmc-ladder: a swap round every E steps (default 1; 0: never)
    --mcmc-post [P ...]       with --mcmc: the posterior summaries are reduced ON THE DEVICE (misti_ensemble_posterior) - without --mcmc-out the
                              chain never leaves it.  In place of the `mcmc:` lines one `post:` line per coordinate: mean, standard
                              deviation, the quantiles P ... (1 ... 8 probabilities in [0, 1]; default 0.025 0.5 0.975; exact order
                              statistics, interpolated), tau, n_eff = samples / tau, `(short)`, the coordinate's row of the correlation
                              matrix, and the best sample
    --mcmc-lag L              with --mcmc-post: the autocorrelation's lag cap (default: every lag)
    --mcmc-hpd [MASS ...]     with --mcmc-post: the SHORTEST (highest-posterior-density) interval of each MASS (1 ... 8 masses in (0, 1];
                              default 0.95) per coordinate, from a full sort of every marginal on the device; each `post:` line gains
                              ` hpd MASS = [lo, hi]` behind its quantiles.  An equal-tailed interval cuts 2.5 % off the low side even where the
                              posterior piles up at the edge of the box; the shortest one does not.  For a --mcmc-log coordinate the ends are
                              printed in natural units, but the interval is the shortest on the log scale: HPD is not invariant under the map
    --mcmc-joint A B [BINS]   with --mcmc; repeatable: the JOINT region of the coordinates A and B (an index, or st - as --box names them), reduced
                              ON THE DEVICE (misti_ensemble_sample_joint): a histogram of BINS x BINS cells (1 ... 128; default 32) over the
                              pair's --box, its mode, and per mass the count level whose cells enclose it - the ridge between a split time and
                              a rate is neither an interval nor an ellipse.  One `joint:` line per fit and pair: the window, the mode cell's
                              centre, and per mass `level`, `cells`, `held / inside` and the extent per axis.  Works with and without
                              --mcmc-post, --mcmc-ladder, --mcmc-log and --mcmc-prior.  The histogram lives in the SAMPLING coordinate: for a
                              --mcmc-log coordinate the line prints natural units, the IMAGE of a region that is highest-density on the log scale
    --mcmc-joint-mass P ...   with --mcmc-joint: the masses of the regions (1 ... 8, each in (0, 1]; default 0.95)
    --mcmc-joint-out FILE.npz with --mcmc-joint: the counts, ranges, bin edges and levels of every fit and pair, as NumPy arrays
    --mcmc-bands [P ...]      with --mcmc: per fit the BAND of the corrected coalescence rates lc per interval and population (misti_traj_bands) over the
                              kept samples behind the burn-in, in natural units, the split from the fitted coordinate where there is one: `bands:`
                              lines with count / m (the share of samples whose populations are still separate there), lo, the quantiles of each P
                              (default 0.025 0.5 0.975), hi - RATES, not sizes 1 / lc: an interpolated quantile does not map through 1 / x.  The
                              chain is read back for this, as for --mcmc-out; with --mcmc-ladder the cold rung's
    --mcmc-bands-thin T       with --mcmc-bands: every T-th kept step (default 1)
    --bands [P ...]           with --all-bs and --grid-solve or --fit-st (with or without --hops, --de, --box): the same band over the bootstrap
                              rows' fits - under --grid-solve each row at its best split; row 0, the point estimate, is reported beside it
                              (`bands: point` lines) - a `bands:` line per interval below the largest fitted split
    --bands-out FILE.npz      with --bands: count, mean, quant, lo, hi, probs, the point estimate's rates and the fits, as NumPy arrays
    --mcmc-log K [K ...]      with --mcmc: coordinate K (an index, or st - as --box names them) is SAMPLED ON THE LOG SCALE (misti_ensemble_sample_prior):
                              the stretch, the box test and the chain are in ln(value), the engine is handed the value.  Its --box is given in
                              natural units and needs LO > 0; flat on the log scale is the log-uniform prior.  The `mcmc:` / `post:` lines print
                              quantiles and the best sample in natural units and the mean (sd) of the logarithm, and say so
    --mcmc-prior K normal MEAN SD | K exponential SCALE
                              with --mcmc: a prior on coordinate K's SAMPLING coordinate (repeatable) - on a --mcmc-log coordinate a normal is a
                              log-normal; the exponential is measured from the box's lower bound.  Not tempered by --mcmc-temp / --mcmc-ladder
    --box K LO HI             with --grid-solve, --fit-st or --polish, with or without --hops; repeatable: every search runs inside a box -
                              SciPy's Nelder-Mead with bounds= (misti_nm_solve_box / misti_basinhopping_box): LO <= parameter K <= HI, K the
                              index of an optimised parameter as --grid-mi K names it, or `st` for the fitted split of --fit-st.  inf and
                              -inf are accepted, LO = HI holds the coordinate fixed, a coordinate without a --box is unbounded; a start
                              outside the box is clipped into it.  Refused anywhere else, and `st` without --fit-st
    --top K                   with --grid-st and/or --grid-mi (K = 1 ... 8): grid mode evaluates WITHOUT replicates and reduces on the device
                              (misti_scan_best_dev) - the [candidates x rows] likelihood table is never made; per row its K best
                              candidates are printed (one line each, grid mode's format: K lines per row in place of one per
                              candidate), then the best: line, the bootstrap interval from the rows' first places and the timing line.
                              Not offered with --gpus N > 1, --devices, --grid-solve, --fit-st, --sweep or --sweep-pu
    --polish                  with --top K and at least one optimised -mi / -pu: after the scan ONE batched search whose starts are
                              the K listed candidates of every row (optimize.scan_polish); per row the MiSTI.py:240 line of its
                              best polished search, as --grid-solve prints its pairs - K searches per row where --grid-solve runs
                              one from every (split, start) pair
    --profile AXIS [AXIS]     with --grid-st and/or --grid-mi: the PROFILE likelihood along one scanned axis, or the surface over two -
                              AXIS is `st` or the index K of an optimised parameter as --grid-mi K names it.  Grid mode evaluates
                              WITHOUT replicates and reduces on the device (misti_scan_profile_dev; the table is never made): per row
                              and per value of the axis one line with the best llh over every other scanned quantity and the candidate
                              that attains it, then the best: line, for one axis a support: line per row (the axis values within
                              --profile-drop D of the row's maximum; D defaults to half the 95 % point of chi-square with one degree of
                              freedom - a likelihood-ratio support interval of a composite likelihood, not a confidence interval), with
                              --all-bs and axis st the bootstrap interval, and the timing line.  Not offered with --top, --polish,
                              --fit-st, --grid-solve, --sweep, --sweep-pu, --gpus N > 1 or --devices
    --se                      with --grid-solve (also with --all-bs) or with the plain single-model Solve: after the fit, the curvature
                              of the log-likelihood at every fitted point (misti_curvature: one stencil of 1 + 2 n^2 evaluations per
                              point, the split held fixed) - per fitted rate the standard error from the observed information
                              inv(-H), the correlation matrix and the condition number of -H, one `se:` line per printed fit; a fit
                              whose -H is not positive definite (a flat direction, a rate on its boundary) says so instead.  With at
                              least three bootstrap rows (--all-bs, or -bs N on a file of 1 + B rows: row 0 is the data, the rest
                              resamples) also the sandwich standard error H^-1 (A C A^T) H^-1 of a composite likelihood, C the
                              covariance of the class counts over those rows.  Not offered with --gpus N > 1, --devices, --fit-st,
                              --hops, --sweep or --sweep-pu; grid mode needs --grid-solve for it.  Every other line stays as it is
    --se-step REL             with --se (refused without): the relative step of the stencil, h_i = REL x |rate_i|, adjusted by at most
                              half an ulp of the rate so that rate +- h_i are exact (default 1e-2:
                              DESIGN.md section 4 measures it; a rate near zero needs an absolute step)
    --gpus N                  the sweep on N GPUs of the node: this process starts N ranks (one per GPU, torch.distributed over
                              RCCL), whole lambda-correction chains are dealt to the ranks, one all_gather, rank 0 prints
    --devices 0,1,...         the sweep on a LIST of devices from this one process (misti_create_multi: one context and one host
                              thread per entry)
    --sweep NAME V1 V2 ...    the recipe's `::: NAME V1 V2 ...` (repeatable): {NAME} stands in the positional split time and in the
                              start, end and rate fields of -mi (misti_amd/sweep.py).  Without --grid-solve (every -mi / -pu fixed,
                              flag 0: an optimised one is refused, the reference would fit it) every model of the product (first
                              sweep outermost) times the JSFS rows (-bs N or --all-bs) is evaluated in ONE batch with per-candidate
                              band bounds, and every model prints the MiSTI.py:240 line; with --grid-solve (required as soon as a
                              parameter is optimised) the time
                              variables make the models, the rate variables of optimised bands the starts, and every (row, model)
                              pair is optimised in ONE batched search (misti_nm_solve_bounds)
    --sweep-pu NAME V1 V2 ... a sweep variable of the pulses (repeatable): {NAME} stands in the time field or in the fraction field
                              of -pu - `-pu 2 {t} {f} 0`, "when did the admixture pulse happen".  The models are the product of the
                              --sweep variables, then the --sweep-pu variables (last innermost); every batch carries per-candidate
                              pulse times (misti_eval_batch_pulses; with --grid-solve misti_nm_solve_pulses, the fractions of an
                              optimised pulse being the starts)
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from math import ceil

import numpy as np

from . import io as mio
from .engine import BatchResult, Engine, MigrationInference
from .sweep import split_arg, sweep_error


RANK_MODULE = "misti_amd.cli"       # what `--gpus N` starts N times (a test driver that wraps this module names itself here)


def build_parser():
    p = argparse.ArgumentParser(description="Migration inference from PSMC (MI355X engine).")
    p.add_argument("fpsmc1", help="psmc file 1")
    p.add_argument("fpsmc2", help="psmc file 2")
    p.add_argument("fjafs", help="joint allele frequency spectrum file")
    p.add_argument("st", type=split_arg, help="split time (or {NAME} of a --sweep)")
    p.add_argument("-o", "--fout", default="", help="output file, default is stdout")
    p.add_argument("-wd", default="", help="working directory (path to data files)")
    p.add_argument("-tol", type=float, default=1e-4, help="optimisation precision (default is 1e-4)")
    p.add_argument("-mth", type=float, default=0.0, help="mixture treshhold (default is 0.0)")
    p.add_argument("-mi", nargs=5, action="append", default=[],
                   help="migration rate: source population (1 or 2), start, end, initial value, fixed(0)/optimised(1)")
    p.add_argument("-pu", nargs=4, action="append", default=[],
                   help="pulse migration: source population (1 or 2), time, rate, fixed(0)/optimised(1)")
    p.add_argument("--sdate", type=float, default=0, help="dating of the second sample (for ancient genome)")
    p.add_argument("--hetloss", "-hl", nargs=2, type=float, help="loss of heterozygosity for the two genomes")
    p.add_argument("--discr", "-d", type=int, default=1, help="accepted for compatibility (the reference ignores it)")
    p.add_argument("-rd", type=int, default=-1, help="round (RD) in the PSMC files, -1 = last")
    p.add_argument("--funits", type=str, default="setunits.txt", help="file with units to rescale times and EPS")
    p.add_argument("-uf", action="store_true", help="unfolded spectrum")
    p.add_argument("--nosmooth", action="store_true", help="don't smooth")
    p.add_argument("--trueEPS", action="store_true", help="input is true effective population size")
    p.add_argument("--cpfit", action="store_true", help="fit probabilities to coalesce within each interval")
    p.add_argument("--bsMode", "-bs", type=int, default=-1, help="use JSFS row N (-1: sum of all rows)")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--device", type=int, default=0, help="HIP device index")
    p.add_argument("--grid-st", nargs="+", type=float, metavar="V", help="A B [STEP]: scan split times")
    p.add_argument("--grid-mi", nargs=4, action="append", default=[], metavar=("K", "LO", "HI", "N"),
                   help="log-spaced values for optimised parameter K")
    p.add_argument("--all-bs", action="store_true", help="evaluate every JSFS row as a bootstrap replicate")
    p.add_argument("--bootstrap", type=int, default=None, metavar="N",
                   help="the JSFS rows are chunks: draw N block-bootstrap replicates of them on the device (the project's own counter-based stream, "
                        "not the reference's Mersenne Twister) and evaluate the 1 + N-row table; implies --all-bs")
    p.add_argument("--bs-seed", type=int, default=None, metavar="K", help="with --bootstrap: the seed of the replicates' streams, a uint64 (default 0)")
    p.add_argument("--bs-normalize", action="store_true", help="with --bootstrap: scale every replicate to the data's number of segregating sites")
    p.add_argument("--bootstrap-out", type=str, default=None, metavar="FILE", help="with --bootstrap: write the table that was drawn as a #MiSTI_JSFS file")
    p.add_argument("--parametric", type=int, default=None, metavar="N",
                   help="a JSFS without chunks: fit the data row, then draw N parametric-bootstrap replicates from the fitted spectrum on the device and "
                        "evaluate the 1 + N-row table; implies --all-bs; --bs-seed and --bootstrap-out apply.  The sites are drawn independently, real "
                        "sites are linked: intervals from these replicates are narrower than a block bootstrap's (--bootstrap, where the file has chunks)")
    p.add_argument("--sites", type=int, default=None, metavar="M",
                   help="with --parametric: sites per replicate (default: the data row's number of sites; fewer = an effective number of independent sites)")
    p.add_argument("--jackknife", type=int, default=None, metavar="M",
                   help="with --fit-st / --grid-solve: the JSFS rows are chunks: make the delete-M block jackknife's 1 + G-row table on the device (row 0 the "
                        "sum of all chunks, then the leave-out rows of groups of M chunks) and print jackknife: lines - estimate, bias-corrected estimate, "
                        "bias, standard error, t-interval - for the fitted split and every rate; implies --all-bs; M = 0: the file already is such a table")
    p.add_argument("--jackknife-out", type=str, default=None, metavar="FILE",
                   help="with --jackknife M >= 1: write the table that was made as a #MiSTI_JSFS file (--jackknife 0 --all-bs on it repeats the run)")
    p.add_argument("--gpus", type=int, default=1, help="grid mode: start this many ranks, one per GPU (replaces `parallel -j N ./MiSTI.py ...`)")
    p.add_argument("--devices", type=str, default="", help="grid mode: comma-separated device list evaluated from this one process (misti_create_multi)")
    p.add_argument("--grid-solve", action="store_true",
                   help="with --grid-st / --all-bs: optimise every (replicate, split) pair as the test.bs loops do, in one batched search")
    p.add_argument("--fit-st", action="store_true",
                   help="with --grid-st (the initial splits) / --all-bs: fit the split time per row as a coordinate of one batched search")
    p.add_argument("--hops", type=int, default=None, metavar="N",
                   help="with --fit-st / --grid-solve: basin hopping with N hops (T = 0.5, SciPy's minimiser defaults; -tol does not apply) in place of the local search")
    p.add_argument("--hop-step", type=float, default=None, metavar="S", help="with --hops: initial step size of the random displacement (default 0.5)")
    p.add_argument("--hop-seed", type=int, default=None, metavar="K", help="with --hops: seed of the searches' generators (default 0)")
    p.add_argument("--de", nargs=2, type=int, default=None, metavar=("POP", "GENS"),
                   help="with --fit-st / --grid-solve: differential evolution of POP members over at most GENS generations inside the --box of "
                        "every searched coordinate, in place of the local search (the project's own rule, not SciPy's)")
    p.add_argument("--de-seed", type=int, default=None, metavar="K", help="with --de: seed of the searches' Philox streams (default 0)")
    p.add_argument("--de-F", nargs=2, type=float, default=None, metavar=("LO", "HI"), dest="de_F", help="with --de: dither range of the differential weight (default 0.5 1)")
    p.add_argument("--de-CR", type=float, default=None, metavar="C", dest="de_CR", help="with --de: crossover probability (default 0.7)")
    p.add_argument("--de-polish", action="store_true", help="with --de: one boxed Nelder-Mead call from the DE results; a search keeps the better result")
    p.add_argument("--mcmc", nargs=2, type=int, default=None, metavar=("W", "STEPS"),
                   help="with --fit-st / --grid-solve: after the fit, an ensemble MCMC of W walkers over STEPS steps per printed fit inside the "
                        "--box of every coordinate (the affine-invariant stretch move; the project's own rule)")
    p.add_argument("--mcmc-burn", type=int, default=None, metavar="B", help="with --mcmc: kept steps dropped before the summary (default: half)")
    p.add_argument("--mcmc-thin", type=int, default=None, metavar="K", help="with --mcmc: keep every K-th step (default 1)")
    p.add_argument("--mcmc-seed", type=int, default=None, metavar="K", help="with --mcmc: seed of the ensembles' Philox streams (default 0)")
    p.add_argument("--mcmc-spread", type=float, default=None, metavar="S", help="with --mcmc: spread of the initial ensemble in box widths (default 1e-2)")
    p.add_argument("--mcmc-temp", default=None, metavar="T|auto", help="with --mcmc: the temperature (default 1), or auto: trace(H^-1 J) / p (needs --all-bs)")
    p.add_argument("--mcmc-out", default=None, metavar="FILE.npz", help="with --mcmc: write chains, values, acceptance counters and final ensembles")
    p.add_argument("--mcmc-ladder", nargs=2, default=None, metavar=("L", "RATIO"),
                   help="with --mcmc: parallel tempering, L rungs per fit at T0 RATIO^(l / (L - 1)); `ladder:` lines behind the cold rung's summary")
    p.add_argument("--mcmc-swap", type=int, default=None, metavar="E", help="with --mcmc-ladder: a swap round every E steps (default 1; 0: never)")
    p.add_argument("--mcmc-post", nargs="*", type=float, default=None, metavar="P",
                   help="with --mcmc: posterior summaries reduced on the device, `post:` lines in place of `mcmc:` lines; P ...: the quantiles (default 0.025 0.5 0.975)")
    p.add_argument("--mcmc-joint", nargs="+", action="append", default=None, metavar="A",
                   help="with --mcmc; repeatable: A B [BINS] - the joint region of the coordinates A and B (an index, or st), a BINS x BINS histogram (default 32) "
                        "reduced on the device; one `joint:` line per fit and pair")
    p.add_argument("--mcmc-joint-mass", nargs="+", type=float, default=None, metavar="P", help="with --mcmc-joint: the masses of the regions (default 0.95)")
    p.add_argument("--mcmc-joint-out", default=None, metavar="FILE.npz", help="with --mcmc-joint: write counts, ranges, edges and levels")
    p.add_argument("--mcmc-bands", nargs="*", type=float, default=None, metavar="P",
                   help="with --mcmc: per fit the band of the corrected RATES per interval over the kept samples behind the burn-in (count / m, lo, "
                        "the quantiles of each P, hi per population; default 0.025 0.5 0.975), reduced on the device; `bands:` lines per fit")
    p.add_argument("--mcmc-bands-thin", type=int, default=None, metavar="T", help="with --mcmc-bands: every T-th kept step (default 1)")
    p.add_argument("--bands", nargs="*", type=float, default=None, metavar="P",
                   help="with --all-bs and --grid-solve or --fit-st: the band of the corrected RATES per interval over the bootstrap rows' fits (row 0: "
                        "the point estimate, reported beside it; default 0.025 0.5 0.975), reduced on the device; a `bands:` line per interval")
    p.add_argument("--bands-out", default=None, metavar="FILE.npz", help="with --bands: write count, mean, quant, lo, hi, probs, the point estimate's rates and the fits")
    p.add_argument("--mcmc-log", nargs="+", default=None, metavar="K", help="with --mcmc: coordinates (an index, or st) sampled on the log scale; their --box is in natural units, LO > 0")
    p.add_argument("--mcmc-prior", nargs="+", action="append", default=None, metavar="K",
                   help="with --mcmc: K normal MEAN SD | K exponential SCALE - a prior on coordinate K's sampling coordinate (repeatable)")
    p.add_argument("--mcmc-lag", type=int, default=None, metavar="L", help="with --mcmc-post: the autocorrelation's lag cap (default: every lag)")
    p.add_argument("--mcmc-hpd", nargs="*", type=float, default=None, metavar="MASS",
                   help="with --mcmc-post: the shortest (HPD) interval of each MASS per coordinate, ` hpd MASS = [lo, hi]` on the `post:` lines (default 0.95)")
    p.add_argument("--box", nargs=3, action="append", default=[], metavar=("K", "LO", "HI"),
                   help="with --grid-solve / --fit-st / --polish: keep optimised parameter K (or `st`: the fitted split of --fit-st) within [LO, HI] "
                        "in every search (SciPy's bounds=; inf / -inf accepted); repeatable")
    # `--box K -inf HI`: argparse takes an argument that starts with `-` for an option unless it looks like a negative number (and no
    # option of this parser does); -inf is one
    import re
    p._negative_number_matcher = re.compile(r"^-\d+$|^-\d*\.\d+$|^-inf$")
    p.add_argument("--top", type=int, default=None, metavar="K",
                   help="grid mode (--grid-st / --grid-mi): keep the K best candidates per row (1 ... 8), reduced on the device without the table")
    p.add_argument("--polish", action="store_true",
                   help="with --top K: one batched search from the K listed candidates of every row; per row its best polished search")
    p.add_argument("--profile", nargs="+", default=None, metavar="AXIS",
                   help="grid mode: the profile likelihood per row along one scanned axis (st, or K of --grid-mi K) or over two, reduced on the device without the table")
    p.add_argument("--profile-drop", type=float, default=None, metavar="D",
                   help="with --profile AXIS: the support: line lists the axis values within D of the row's maximum (default: chi2.ppf(0.95, 1) / 2)")
    p.add_argument("--se", action="store_true",
                   help="with --grid-solve or the single-model Solve: standard errors and correlations of the fitted rates from the Hessian at the fit "
                        "(and the sandwich standard error with at least three bootstrap rows)")
    p.add_argument("--se-step", type=float, default=None, metavar="REL", help="with --se: relative step of the stencil (default 1e-2)")
    p.add_argument("--sweep", nargs="+", action="append", default=[], metavar=("NAME", "V"),
                   help="the GNU-parallel recipe's `::: NAME V1 V2 ...`: {NAME} in the split time or in -mi start / end / rate fields")
    p.add_argument("--sweep-pu", nargs="+", action="append", default=[], metavar=("NAME", "V"),
                   help="a sweep variable of the pulses: {NAME} in the time field or in the fraction field of -pu")
    return p


def bootstrap_error(a):
    """Why ``--bootstrap`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if a.bootstrap is None:
        if getattr(a, "parametric", None) is not None:
            return None                                     # --bs-seed / --bootstrap-out belong to --parametric too: parametric_error
        if a.bs_seed is not None or a.bs_normalize or a.bootstrap_out is not None:
            return "--bs-seed / --bs-normalize / --bootstrap-out belong to --bootstrap N: give --bootstrap N"
        return None
    if a.bootstrap < 1:
        return "--bootstrap N: the number of replicates must be at least 1 (got %d)" % a.bootstrap
    if a.bsMode != -1:
        return "--bootstrap replaces the rows of the file by the table it draws and evaluates every row: -bs K is not offered with it"
    if a.bs_seed is not None and not 0 <= a.bs_seed < 1 << 64:
        return "--bs-seed is a uint64: 0 ... 2^64 - 1 (got %d)" % a.bs_seed
    return None


def bootstrap_rows(a, inp, rows, pop1=None, pop2=None):
    """The table of ``--bootstrap N``: the file's rows are the chunks, the device draws the replicates (Engine.bootstrap_table on this
    process's device - a rank of --gpus N regenerates the same table from (seed, r)); with --bootstrap-out the table is written through
    the JSFS writer (by rank 0)."""
    from .dist import env_rank
    rank, local, world = env_rank()
    device = local if world > 1 else (int(a.devices.split(",")[0]) if a.devices else a.device)
    with Engine(inp.times, inp.lambdas, device=device) as e:
        table = e.bootstrap_table(rows, a.bootstrap, seed=a.bs_seed or 0, normalize=a.bs_normalize)
    table = table.tolist()
    if a.bootstrap_out is not None and rank == 0:
        with open(os.path.join(a.wd, a.bootstrap_out), "w") as fw:
            fw.write(mio.format_jsfs(table, pop1, pop2))
    return table


def parametric_error(a):
    """Why ``--parametric`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if a.parametric is None:
        return "--sites belongs to --parametric N: give --parametric N" if a.sites is not None else None
    if a.parametric < 1:
        return "--parametric N: the number of replicates must be at least 1 (got %d)" % a.parametric
    if a.bootstrap is not None:
        return "--parametric draws its replicates from a fitted spectrum, --bootstrap resamples the chunks of the file: give one of them"
    if a.bs_normalize:
        return "--bs-normalize is not offered with --parametric: every replicate has exactly the number of sites asked for, there is nothing to normalise"
    if a.bsMode != -1:
        return "--parametric replaces the rows of the file by the table it draws and evaluates every row: -bs K is not offered with it"
    if a.bs_seed is not None and not 0 <= a.bs_seed < 1 << 64:
        return "--bs-seed is a uint64: 0 ... 2^64 - 1 (got %d)" % a.bs_seed
    if a.sites is not None and not 1 <= a.sites <= 1 << 36:
        return "--sites M: 1 ... 2^36 sites per replicate (got %d)" % a.sites
    if a.sweep or a.sweep_pu:
        return "--parametric fits the model of this command line at its split time: a {NAME} of a --sweep has no single fit to draw from"
    return None


def parametric_rows(a, inp, data_row, pop1=None, pop2=None):
    """The table of ``--parametric N``.  Stage 1: the ordinary fit of ``data_row`` at the command line's split and initial values (the
    single-model path of main: MigrationInference.Solve), printed as that path prints it.  Stage 2: N replicates drawn on this
    process's device from the spectrum at the fit (Engine.parametric_table - a rank of --gpus N fits and regenerates the same table
    from (seed, r) rather than receiving it); with --bootstrap-out the table is written through the JSFS writer (by rank 0).  Returns
    the table as lists, or None where the fit has no value."""
    from .dist import env_rank
    rank, local, world = env_rank()
    device = local if world > 1 else (int(a.devices.split(",")[0]) if a.devices else a.device)
    times = list(inp.times)                                 # MigrationInference extends its grid in place for a fractional split
    mig = MigrationInference(times, [list(l) for l in inp.lambdas], data_row, a.st, a.mi, a.pu, thrh=[inp.theta, inp.rho], Tpsmc=inp.Tpsmc,
                             enableOutput=False, smooth=not a.nosmooth, unfolded=a.uf, trueEPS=a.trueEPS, sampleDate=inp.sampleDateDiscr,
                             mixtureTH=a.mth, cpfit=a.cpfit, device=device)
    try:
        sol = mig.Solve(a.tol)
        print(sol)
        print("\nParameter estimates:")
        print(result_line(a.bsMode, a.st, times, inp.scaleTime, a.mi, sol[0], sol[1]))
        if sol[1] == -10 ** 9 or not np.isfinite(sol[1]):
            return None
        n_sites = a.sites if a.sites is not None else int(np.rint(np.asarray(data_row[1:], dtype=float).sum()))
        table = mig._engine.parametric_table(a.st, [float(v) for v in sol[0]], data_row, a.parametric, n_sites=n_sites, seed=a.bs_seed or 0)
    finally:
        mig._engine.close()
    print("Parametric bootstrap: %d replicates of %d sites drawn on the device from the spectrum at splitT = %s, optim = [%s] (llh = %s), seed %d: "
          "independent sites - intervals from them are narrower than a block bootstrap's"
          % (a.parametric, n_sites, a.st, ", ".join(str(v) for v in sol[0]), sol[1], a.bs_seed or 0))
    table = table.tolist()
    if a.bootstrap_out is not None and rank == 0:
        with open(os.path.join(a.wd, a.bootstrap_out), "w") as fw:
            fw.write(mio.format_jsfs(table, pop1, pop2))
    return table


JACKKNIFE_NEEDS_A_FIT = "the arg-max over a grid does not move when one block is left out; fit with --fit-st or --grid-solve"


def jackknife_error(a):
    """Why ``--jackknife`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if a.jackknife is None:
        return "--jackknife-out keeps the table of --jackknife M: give --jackknife M with M >= 1" if a.jackknife_out is not None else None
    if a.jackknife < 0:
        return "--jackknife M: the group size must not be negative (got %d; 0: the file already is a jackknife table)" % a.jackknife
    if a.jackknife_out is not None and a.jackknife < 1:
        return "--jackknife-out keeps the table --jackknife M makes: with --jackknife 0 nothing is made - give M >= 1"
    if a.bootstrap is not None or a.parametric is not None:
        return "--jackknife leaves blocks out, --bootstrap / --parametric draw replicates: give one of them"
    if a.bsMode != -1:
        return "--jackknife replaces the rows of the file by its table and fits every row: -bs K is not offered with it"
    if a.se:
        return "--jackknife states its own standard error from the leave-out fits: --se is not offered with it"
    if a.top is not None or a.polish or a.profile is not None or a.sweep or a.sweep_pu or not (a.fit_st or a.grid_solve):
        return "--jackknife: " + JACKKNIFE_NEEDS_A_FIT
    return None


def jackknife_rows(a, inp, rows, pop1=None, pop2=None):
    """The table of ``--jackknife M``: the file's rows are the chunks, the device makes the leave-out rows (Engine.jackknife_table on this
    process's device - a rank of --gpus N makes the same table itself: it depends on the chunks and M alone); with --jackknife-out the
    table is written through the JSFS writer (by rank 0)."""
    from .dist import env_rank
    rank, local, world = env_rank()
    device = local if world > 1 else (int(a.devices.split(",")[0]) if a.devices else a.device)
    with Engine(inp.times, inp.lambdas, device=device) as e:
        table = e.jackknife_table(rows, a.jackknife)
    table = table.tolist()
    if a.jackknife_out is not None and rank == 0:
        with open(os.path.join(a.wd, a.jackknife_out), "w") as fw:
            fw.write(mio.format_jsfs(table, pop1, pop2))
    return table


def print_jackknife(names, theta, lengths):
    """The ``jackknife:`` lines: per named quantity (``theta[1 + G][K]``: row 0's estimate, then the leave-out rows'; NaN where a row
    has no fit) the weighted delete-m jackknife of optimize.jackknife_estimate, weighted by ``lengths`` - column 0 of the table.
    Numbers are printed with repr: they read back exactly."""
    from .optimize import jackknife_estimate
    try:
        est = jackknife_estimate(np.asarray(theta, dtype=float).reshape(len(lengths), len(names)), lengths)
    except ValueError as e:
        print("jackknife: no interval:", e)
        return
    for k, name in enumerate(names):
        if not np.isfinite(est["estimate"][k]):
            print("jackknife:", name, "\tbs_id = 0 has no fit: no estimate")
        elif est["n_group"][k] < 2:
            print("jackknife:", name, "\tno interval (%d leave-out rows with a fit; at least 2 needed)" % est["n_group"][k])
        else:
            print("jackknife:", name, "\testimate = %r \tjackknife = %r \tbias = %r \tse = %r \tinterval = [%r, %r] \tgroups = %d"
                  % (float(est["estimate"][k]), float(est["jackknife"][k]), float(est["bias"][k]), float(est["se"][k]),
                     float(est["interval"][k, 0]), float(est["interval"][k, 1]), int(est["n_group"][k])))


def se_error(a):
    """Why ``--se`` / ``--se-step`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if not a.se:
        if a.se_step is not None:
            return "--se-step sets the stencil's step of --se: give --se"
        return None
    if a.sweep or a.sweep_pu:
        return "--se reports the curvature at the fit of ONE model: --sweep / --sweep-pu are not offered with it"
    if a.gpus > 1 or a.devices:
        return "--se runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    if a.fit_st:
        return "--se holds the split time fixed (the objective is piecewise in it): --fit-st is not offered with it"
    if a.hops is not None:
        return "--se follows the local search of --grid-solve or of the single model: --hops is not offered with it"
    if not a.grid_solve and (a.grid_st or a.grid_mi or a.all_bs or a.top is not None or a.profile is not None):
        return "--se reports the curvature at a FITTED point: with --grid-st / --grid-mi / --all-bs it needs --grid-solve"
    if a.se_step is not None and not (a.se_step > 0 and np.isfinite(a.se_step)):
        return "--se-step must be positive and finite (got %g)" % a.se_step
    if not any(int(el[4]) for el in a.mi) and not any(int(el[3]) for el in a.pu):
        return "--se needs at least one optimised parameter (-mi ... 1 or -pu ... 1)"
    return None


def _se_step(a):
    """--se-step, or its default: optimize.CURV_REL_STEP (1e-2; measured in DESIGN.md section 4)."""
    from .optimize import CURV_REL_STEP
    return CURV_REL_STEP if a.se_step is None else a.se_step


def print_se(labels, cur, table=None, unfolded=False):
    """The ``se:`` lines of --se: per fitted point (``labels[p]``: what names it, ``cur``: Engine.curvature at the fits) the standard
    errors from the observed information, the correlation matrix and the condition number of -H; with ``table`` (row 0 the data,
    at least three bootstrap rows behind it) the sandwich standard errors as well.  Numbers are printed with repr: they read back exactly."""
    from .optimize import correlation, observed_covariance, sandwich_covariance, standard_errors
    obs = observed_covariance(cur.hess)
    se, corr = standard_errors(obs["cov"]), correlation(obs["cov"])
    sand = standard_errors(sandwich_covariance(cur.hess, cur.dlog, table, unfolded=unfolded)) if table is not None else None
    vec = lambda v: "[" + ", ".join(repr(float(t)) for t in v) + "]"
    for p, label in enumerate(labels):
        if cur.status[p] == 7:
            print("se:", label, "\tno two-sided stencil: a fitted rate lies within its step of 0 (status 7)")
        elif cur.status[p] != 0:
            print("se:", label, "\tno value at a stencil point (status %d)" % int(cur.status[p]))
        elif not obs["ok"][p]:
            print("se:", label, "\t-H is not positive definite (eigenvalues %s): no standard error - a flat direction or a point that is no maximum"
                  % vec(obs["eigenvalues"][p]))
        else:
            print("se:", label, "\tse =", vec(se[p]), "\tcorr =", "[" + ", ".join(vec(r) for r in corr[p]) + "]", "\tcond = %.6g" % obs["cond"][p],
                  ("\tsandwich se = " + vec(sand[p])) if sand is not None else "")


def grid_solve_error(a):
    """Why ``--grid-solve`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if not a.grid_solve:
        return None
    if not (a.grid_st or a.all_bs or a.sweep or a.sweep_pu):
        return "--grid-solve optimises every (replicate, split) pair: it needs --grid-st and/or --all-bs"
    if a.gpus > 1 or a.devices:
        return "--grid-solve runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    if not (a.sweep or a.sweep_pu) and not any(int(el[4]) for el in a.mi) and not any(int(el[3]) for el in a.pu):
        return "--grid-solve needs at least one optimised parameter (-mi ... 1 or -pu ... 1)"
    return None


def fit_st_error(a):
    """Why ``--fit-st`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if not a.fit_st:
        return None
    if a.sweep or a.sweep_pu:
        return "--fit-st fits the split time of ONE model: --sweep / --sweep-pu are not offered with it"
    if a.gpus > 1 or a.devices:
        return "--fit-st runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    if a.grid_solve:
        return "--fit-st fits the split time, --grid-solve scans it: give one of them"
    if not a.grid_st:
        return "--fit-st needs --grid-st A B [STEP]: the initial split times of its searches"
    return None


def hops_error(a):
    """Why ``--hops`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if a.hops is None:
        if a.hop_step is not None or a.hop_seed is not None:
            return "--hop-step / --hop-seed set the hops of --hops N: give --hops N"
        return None
    if a.hops < 1:
        return "--hops N: the number of hops must be at least 1 (got %d)" % a.hops
    if a.sweep or a.sweep_pu:
        return "--hops searches ONE model globally: --sweep / --sweep-pu are not offered with it"
    if not (a.fit_st or a.grid_solve):
        return "--hops makes the searches of --fit-st or --grid-solve global: give one of them"
    if a.gpus > 1 or a.devices:
        return "--hops runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    if a.hop_step is not None and not a.hop_step > 0:
        return "--hop-step must be positive (got %g)" % a.hop_step
    if a.hop_seed is not None and a.hop_seed < 0:
        return "--hop-seed must not be negative (got %d)" % a.hop_seed
    return None


def de_error(a):
    """Why ``--de`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if a.de is None:
        if a.de_seed is not None or a.de_F is not None or a.de_CR is not None or a.de_polish:
            return "--de-seed / --de-F / --de-CR / --de-polish set the search of --de POP GENS: give --de POP GENS"
        return None
    pop, gens = a.de
    if not 4 <= pop <= 256:
        return "--de POP GENS: POP must be 4 ... 256 (got %d)" % pop
    if gens < 1:
        return "--de POP GENS: GENS must be at least 1 (got %d)" % gens
    if a.hops is not None:
        return "--de and --hops are two global searches: give one of them"
    if a.se:
        return "--se follows the local search of --grid-solve or of the single model: --de is not offered with it"
    if a.sweep or a.sweep_pu:
        return "--de searches ONE model globally: --sweep / --sweep-pu are not offered with it"
    if not (a.fit_st or a.grid_solve):
        return "--de makes the searches of --fit-st or --grid-solve global: give one of them"
    if a.gpus > 1 or a.devices:
        return "--de runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    if a.grid_mi:
        return "--de draws its population inside the box: --grid-mi starts are not offered with it (member 0 is the -mi/-pu initial values)"
    if a.de_seed is not None and not 0 <= a.de_seed < 2 ** 64:
        return "--de-seed must be a uint64 (got %d)" % a.de_seed
    if a.de_F is not None and not (0 <= a.de_F[0] <= a.de_F[1] and np.isfinite(a.de_F[1])):
        return "--de-F LO HI: a finite range 0 <= LO <= HI (got %g %g)" % tuple(a.de_F)
    if a.de_CR is not None and not 0 <= a.de_CR <= 1:
        return "--de-CR must lie in [0, 1] (got %g)" % a.de_CR
    k = sum(1 for el in a.mi if int(el[4])) + sum(1 for el in a.pu if int(el[3]))
    boxed = {}
    for name, lo, hi in a.box:
        try:
            boxed[name] = (float(lo), float(hi))
        except ValueError:
            return None                                   # box_error names it
    for name in [str(i) for i in range(k)] + (["st"] if a.fit_st else []):
        if name not in boxed:
            return "--de searches inside a box: coordinate %s has no --box %s LO HI" % (name, name)
        if not all(np.isfinite(v) for v in boxed[name]):
            return "--de needs a finite box: --box %s has an infinite bound" % name
    return None


def mcmc_error(a):
    """Why ``--mcmc`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if a.mcmc is None:
        if a.mcmc_post is not None or a.mcmc_lag is not None:
            return "--mcmc-post / --mcmc-lag summarise the chains of --mcmc W STEPS: give --mcmc W STEPS"
        if a.mcmc_hpd is not None:
            return "--mcmc-hpd gives the shortest intervals of --mcmc W STEPS --mcmc-post: give --mcmc W STEPS"
        if any(v is not None for v in (a.mcmc_burn, a.mcmc_thin, a.mcmc_seed, a.mcmc_spread, a.mcmc_temp, a.mcmc_out)):
            return "--mcmc-burn / --mcmc-thin / --mcmc-seed / --mcmc-spread / --mcmc-temp / --mcmc-out set the sampler of --mcmc W STEPS: give --mcmc W STEPS"
        if a.mcmc_ladder is not None or a.mcmc_swap is not None:
            return "--mcmc-ladder / --mcmc-swap temper the sampler of --mcmc W STEPS: give --mcmc W STEPS"
        if a.mcmc_log is not None or a.mcmc_prior is not None:
            return "--mcmc-log / --mcmc-prior state the coordinates and priors of --mcmc W STEPS: give --mcmc W STEPS"
        if a.mcmc_joint is not None or a.mcmc_joint_mass is not None or a.mcmc_joint_out is not None:
            return "--mcmc-joint / --mcmc-joint-mass / --mcmc-joint-out give the joint regions of --mcmc W STEPS: give --mcmc W STEPS"
        if a.mcmc_bands is not None or a.mcmc_bands_thin is not None:
            return "--mcmc-bands / --mcmc-bands-thin give the trajectory bands of --mcmc W STEPS: give --mcmc W STEPS"
        return None
    W, steps = a.mcmc
    if not 4 <= W <= 256 or W % 2:
        return "--mcmc W STEPS: W must be even, 4 ... 256 (got %d)" % W
    if steps < 1:
        return "--mcmc W STEPS: STEPS must be at least 1 (got %d)" % steps
    if not (a.fit_st or a.grid_solve):
        return "--mcmc samples around the fits of --fit-st or --grid-solve: give one of them"
    if a.se:
        return "--se and --mcmc are two answers to one question: give one of them (--mcmc-temp auto takes the curvature itself)"
    if a.sweep or a.sweep_pu:
        return "--mcmc samples ONE model: --sweep / --sweep-pu are not offered with it"
    if a.gpus > 1 or a.devices:
        return "--mcmc runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    thin = 1 if a.mcmc_thin is None else a.mcmc_thin
    if thin < 1 or steps // thin < 1:
        return "--mcmc-thin K: 1 <= K <= STEPS (got %d)" % thin
    if a.mcmc_burn is not None and not 0 <= a.mcmc_burn < steps // thin:
        return "--mcmc-burn B: 0 <= B < %d kept steps (got %d)" % (steps // thin, a.mcmc_burn)
    if a.mcmc_seed is not None and not 0 <= a.mcmc_seed < 2 ** 64:
        return "--mcmc-seed must be a uint64 (got %d)" % a.mcmc_seed
    if a.mcmc_spread is not None and not (np.isfinite(a.mcmc_spread) and a.mcmc_spread >= 0):
        return "--mcmc-spread must be finite and not negative (got %g)" % a.mcmc_spread
    if a.mcmc_temp is not None and a.mcmc_temp != "auto":
        try:
            T = float(a.mcmc_temp)
        except ValueError:
            T = float("nan")
        if not (np.isfinite(T) and T > 0):
            return "--mcmc-temp T|auto: a finite temperature > 0, or auto (got %s)" % a.mcmc_temp
    if a.mcmc_temp == "auto" and not a.all_bs:
        return "--mcmc-temp auto takes the score covariance from the bootstrap rows: it needs --all-bs"
    if a.mcmc_post is not None and (len(a.mcmc_post) > 8 or not all(0.0 <= v <= 1.0 for v in a.mcmc_post)):
        return "--mcmc-post [P ...]: at most 8 probabilities, each in [0, 1] (got %s)" % " ".join("%g" % v for v in a.mcmc_post)
    if a.mcmc_lag is not None and (a.mcmc_post is None or a.mcmc_lag < 0):
        return "--mcmc-lag L caps the lags of --mcmc-post: give --mcmc-post, and L >= 0"
    if a.mcmc_hpd is not None and a.mcmc_post is None:
        return "--mcmc-hpd [MASS ...] adds the shortest intervals to the summaries of --mcmc-post: give --mcmc-post"
    if a.mcmc_hpd is not None and (len(a.mcmc_hpd) > 8 or not all(0.0 < v <= 1.0 for v in a.mcmc_hpd)):
        return "--mcmc-hpd [MASS ...]: at most 8 masses, each in (0, 1] (got %s)" % " ".join("%g" % v for v in a.mcmc_hpd)
    if a.mcmc_swap is not None and (a.mcmc_ladder is None or a.mcmc_swap < 0):
        return "--mcmc-swap E sets the swap rounds of --mcmc-ladder: give --mcmc-ladder, and E >= 0"
    if a.mcmc_ladder is not None:
        try:
            L, ratio = int(a.mcmc_ladder[0]), float(a.mcmc_ladder[1])
        except ValueError:
            return "--mcmc-ladder L RATIO: an integer and a number (got %s %s)" % tuple(a.mcmc_ladder)
        if not 1 <= L <= 64:
            return "--mcmc-ladder L RATIO: 1 <= L <= 64 rungs (got %d)" % L
        if L > 1 and not (np.isfinite(ratio) and ratio > 1.0):
            return "--mcmc-ladder L RATIO: RATIO must be finite and > 1 (got %s)" % a.mcmc_ladder[1]
    k = sum(1 for el in a.mi if int(el[4])) + sum(1 for el in a.pu if int(el[3]))
    boxed = {}
    for name, lo, hi in a.box:
        try:
            boxed[name] = (float(lo), float(hi))
        except ValueError:
            return None                                   # box_error names it
    for name in [str(i) for i in range(k)] + (["st"] if a.fit_st else []):
        if name not in boxed:
            return "--mcmc samples a uniform prior on a box: coordinate %s has no --box %s LO HI" % (name, name)
        if not all(np.isfinite(v) for v in boxed[name]):
            return "--mcmc needs a finite box: --box %s has an infinite bound" % name
    names = [str(i) for i in range(k)] + (["st"] if a.fit_st else [])
    if a.mcmc_joint is None and (a.mcmc_joint_mass is not None or a.mcmc_joint_out is not None):
        return "--mcmc-joint-mass / --mcmc-joint-out belong to --mcmc-joint A B [BINS]: give it"
    for spec in a.mcmc_joint or ():
        text = " ".join(spec)
        if not 2 <= len(spec) <= 3:
            return "--mcmc-joint A B [BINS]: two coordinates and at most a bin count (got %s)" % text
        for name in spec[:2]:
            if name not in names:
                return "--mcmc-joint %s: %s is no coordinate of this run (%s)" % (text, name, ", ".join(names))
        if spec[0] == spec[1]:
            return "--mcmc-joint %s: A == B - a pair needs two distinct coordinates" % text
        if len(spec) == 3 and not (spec[2].isdigit() and 1 <= int(spec[2]) <= 128):
            return "--mcmc-joint %s: BINS must be an integer, 1 ... 128" % text
    if a.mcmc_joint is not None and len(a.mcmc_joint) > 120:
        return "--mcmc-joint: at most 120 pairs (got %d)" % len(a.mcmc_joint)
    if a.mcmc_joint_mass is not None and (len(a.mcmc_joint_mass) > 8 or not all(0.0 < v <= 1.0 for v in a.mcmc_joint_mass)):
        return "--mcmc-joint-mass P ...: at most 8 masses, each in (0, 1] (got %s)" % " ".join("%g" % v for v in a.mcmc_joint_mass)
    if a.mcmc_bands is None and a.mcmc_bands_thin is not None:
        return "--mcmc-bands-thin T belongs to --mcmc-bands [P ...]: give it"
    if a.mcmc_bands is not None and (len(a.mcmc_bands) > 8 or not all(0.0 <= v <= 1.0 for v in a.mcmc_bands)):
        return "--mcmc-bands [P ...]: at most 8 probabilities, each in [0, 1] (got %s)" % " ".join("%g" % v for v in a.mcmc_bands)
    if a.mcmc_bands_thin is not None and a.mcmc_bands_thin < 1:
        return "--mcmc-bands-thin T: T >= 1 (got %d)" % a.mcmc_bands_thin
    for name in a.mcmc_log or ():
        if name not in names:
            return "--mcmc-log K: %s is no coordinate of this run (%s)" % (name, ", ".join(names))
        if not boxed[name][0] > 0:
            return "--mcmc-log %s samples the logarithm: --box %s needs LO > 0 (got %g)" % (name, name, boxed[name][0])
    if a.mcmc_log and len(set(a.mcmc_log)) != len(a.mcmc_log):
        return "--mcmc-log names a coordinate twice"
    seen = set()
    for spec in a.mcmc_prior or ():
        text = " ".join(spec)
        if spec[0] not in names:
            return "--mcmc-prior %s: %s is no coordinate of this run (%s)" % (text, spec[0], ", ".join(names))
        if spec[0] in seen:
            return "--mcmc-prior %s: coordinate %s already has a prior" % (text, spec[0])
        seen.add(spec[0])
        want = {"normal": 2, "exponential": 1}.get(spec[1] if len(spec) > 1 else "")
        if want is None or len(spec) != 2 + want:
            return "--mcmc-prior K normal MEAN SD | K exponential SCALE (got %s)" % text
        try:
            v = [float(t) for t in spec[2:]]
        except ValueError:
            return "--mcmc-prior %s: the parameters must be numbers" % text
        if not (np.isfinite(v).all() and v[-1] > 0):
            return "--mcmc-prior %s: %s" % (text, "MEAN must be finite, SD finite and > 0" if want == 2 else "SCALE must be finite and > 0")
    return None


BANDS_PROBS = (0.025, 0.5, 0.975)


def bands_error(a):
    """Why ``--bands`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if a.bands is None:
        if a.bands_out is not None:
            return "--bands-out FILE.npz belongs to --bands [P ...]: give it"
        return None
    if not a.all_bs or not (a.fit_st or a.grid_solve):
        return "--bands is the band over the bootstrap rows' fits: it needs --all-bs with --grid-solve or --fit-st"
    if len(a.bands) > 8 or not all(0.0 <= v <= 1.0 for v in a.bands):
        return "--bands [P ...]: at most 8 probabilities, each in [0, 1] (got %s)" % " ".join("%g" % v for v in a.bands)
    if a.sweep or a.sweep_pu:
        return "--bands is the band of ONE model: --sweep / --sweep-pu are not offered with it"
    if a.gpus > 1 or a.devices:
        return "--bands runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    return None


def _probs(given):
    """The probabilities of --bands / --mcmc-bands, or the default where the option stands alone."""
    return tuple(given) if given else BANDS_PROBS


def bands_lines(label, b, times, scale_time, m):
    """The `bands:` lines of one group ``b`` (count[numT][2], lo, quant, hi): per interval with a member its index, its lower edge
    (scaled as the result lines), and per population count / m, lo, the quantiles, hi - RATES, not sizes; %r, so the text carries the bits."""
    from .optimize import trajectory_bands_table
    out = []
    for row in trajectory_bands_table(b, np.cumsum(np.asarray(times, dtype=float))):      # the grid is given as interval lengths
        pops = " \t".join("pop%d: %d/%d lo = %r q = [%s] hi = %r" % (p + 1, row["count"][p], m, float(row["lo"][p]),
                                                                    ", ".join(repr(float(v)) for v in row["quant"][p]), float(row["hi"][p])) for p in (0, 1))
        out.append("bands: %s \tinterval = %d \ttime = %r \t%s" % (label, row["interval"], float(row["time"] * scale_time), pops))
    return out


def _captured(fun, *args):
    """What ``fun`` prints, as text: the engine is open while the band is reduced, the lines belong behind the fits'."""
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fun(*args)
    return buf.getvalue().rstrip("\n")


def run_bands(a, e, x, split, inp):
    """--bands behind the fits ``x[R][k]`` and ``split[R]`` of the R rows of --all-bs: rows 1 ... R - 1 are the samples of ONE group
    (a row without a value: a split of -1, an empty slot to the engine and a member of nothing), row 0 the point estimate, whose own
    rates are reported beside the band.  Prints the `bands:` lines below the largest fitted split and writes --bands-out."""
    probs = _probs(a.bands)
    x, split = np.asarray(x, dtype=float).reshape(len(split), e.n_param), np.asarray(split, dtype=float).copy()
    bad = ~(np.isfinite(split) & np.isfinite(x).all(axis=1))
    split[bad] = -1.0
    x = np.where(bad[:, None], 0.0, x)
    m = len(split) - 1
    point = e.trajectory_bands(x[:1], split[:1], groups=1, probs=(0.5,), want=("count", "lo"))
    rate = np.where(point["count"][0] > 0, point["lo"][0], np.nan)
    print("bands: rates per interval over the fits of %d bootstrap rows (RATES lc, not sizes 1 / lc), probabilities %s" % (m, " ".join("%g" % v for v in probs)))
    for j in np.flatnonzero(point["count"][0].any(axis=1)):
        print("bands: point \tinterval = %d \ttime = %r \tpop1: %r \tpop2: %r" % (j, float(sum(inp.times[:j]) * inp.scaleTime), float(rate[j, 0]), float(rate[j, 1])))
    b = None
    if m >= 1:
        b = e.trajectory_bands(x[1:], split[1:], groups=1, probs=probs)
        for line in bands_lines("bootstrap", {k_: v[0] for k_, v in b.items() if k_ != "probs"}, inp.times, inp.scaleTime, m):
            print(line)
    if a.bands_out:
        empty = np.empty((0,))
        np.savez(a.bands_out, probs=np.asarray(probs), point=rate, x=x, split=split, times=np.asarray(inp.times, dtype=float),
                 **{k_: (b[k_][0] if b is not None else empty) for k_ in ("count", "mean", "quant", "lo", "hi")})


def _mcmc_prior(a, k):
    """The prior of --mcmc-log / --mcmc-prior over the k parameters (and the split, with --fit-st) as optimize.prior_spec states it, or
    None without either option."""
    if not (a.mcmc_log or a.mcmc_prior):
        return None
    from .optimize import prior_spec
    at = lambda name: k if name == "st" else int(name)
    specs = [(at(sp[0]), sp[1], [float(t) for t in sp[2:]]) for sp in a.mcmc_prior or ()]
    return prior_spec(k + (1 if a.fit_st else 0), log=[at(n) for n in a.mcmc_log or ()], normal={c: tuple(v) for c, kind, v in specs if kind == "normal"},
                      exponential={c: v[0] for c, kind, v in specs if kind == "exponential"})


def _mcmc_joint(a, k):
    """The ``joint=`` of the samplers for --mcmc-joint / --mcmc-joint-mass over the k parameters (st: coordinate k), or None without
    the option: every window is the pair's --box, in sampling coordinates."""
    if a.mcmc_joint is None:
        return None
    at = lambda name: k if name == "st" else int(name)
    return dict(pairs=[(at(sp[0]), at(sp[1])) for sp in a.mcmc_joint], bins=[[int(sp[2]) if len(sp) == 3 else 32] * 2 for sp in a.mcmc_joint],
                range="box", masses=tuple(a.mcmc_joint_mass) if a.mcmc_joint_mass else (0.95,))


def _mcmc_from_de(a):
    """--de W GENS ran with the sampler's W: the initial ensembles are DE's final populations."""
    return bool(a.mcmc and a.de and a.de[0] == a.mcmc[0])


def _mcmc_options(a):
    """The options of --mcmc, or their defaults: burn half the kept steps, thin 1, seed 0, spread 1e-2, temperature 1."""
    thin = 1 if a.mcmc_thin is None else a.mcmc_thin
    return dict(walkers=a.mcmc[0], n_step=a.mcmc[1], thin=thin, burn=(a.mcmc[1] // thin) // 2 if a.mcmc_burn is None else a.mcmc_burn,
                seed=0 if a.mcmc_seed is None else a.mcmc_seed, spread=1e-2 if a.mcmc_spread is None else a.mcmc_spread,
                temperature="auto" if a.mcmc_temp == "auto" else 1.0 if a.mcmc_temp is None else float(a.mcmc_temp))


def _mcmc_ladder_options(a):
    """The options of --mcmc-ladder: ladder (L, RATIO), or None without it, and swap_every (default 1)."""
    return dict(ladder=None if a.mcmc_ladder is None else (int(a.mcmc_ladder[0]), float(a.mcmc_ladder[1])), swap_every=1 if a.mcmc_swap is None else a.mcmc_swap)


def run_mcmc(a, e, x, r_of, j_of, data, box, split_times, unfolded, population=None):
    """--mcmc behind the fits ``x[S][N]`` (fit s: row ``r_of[s]``, stream ``j_of[s]``; ``split_times[S]``, or None with the split as the
    last coordinate): ONE Engine.ensemble_sample call from ensemble_start around every fit (a fit without a value: the middle of the
    box) - or, with ``population[S][W][N]`` (``--de W GENS`` ran with the sampler's W), from DE's final populations: dispersed,
    inside the box and already evaluated.  With --mcmc-ladder L RATIO: ONE Engine.tempered_sample call on temperature_ladder(T, RATIO, L),
    every rung from that initial ensemble; the result's ``ladder`` holds the temperatures.
    Returns (options, temperature, result) - or a string: why --mcmc-temp auto has no temperature."""
    from .optimize import composite_temperature, ensemble_start, score_covariance, temperature_ladder, to_sampling
    o = dict(_mcmc_options(a), **_mcmc_ladder_options(a))
    lo, hi = box
    x = np.where(np.isfinite(x), np.clip(x, lo, hi), 0.5 * (lo + hi))
    prior = o["prior"] = _mcmc_prior(a, x.shape[1] - (1 if split_times is None else 0))
    o["fit_split"] = split_times is None
    T = o["temperature"]
    if T == "auto":
        P = e.n_param
        if not P:
            return "--mcmc-temp auto: the model has no optimised parameter, so no curvature"
        if data.shape[0] < 3:
            return "--mcmc-temp auto: the score covariance needs at least two bootstrap rows behind the data row"
        first = int(np.flatnonzero(np.asarray(r_of) == 0)[0])
        cur = e.curvature(x[first:first + 1, :P], [float(split_times[first]) if split_times is not None else float(x[first, -1])], [0], data)
        if cur.status[0] != 0:
            return "--mcmc-temp auto: no curvature at the data row's fit (status %d)" % int(cur.status[0])
        try:
            T = composite_temperature(cur.hess[0], score_covariance(cur.dlog, data, unfolded=unfolded)[0])
        except ValueError as why:
            return "--mcmc-temp auto: %s" % why
    if prior is not None:
        # everything from here on is in sampling coordinates: the box of a --mcmc-log coordinate is the logarithm of its --box, the fits
        # and DE's population are mapped with to_sampling (and clipped: a logarithm may land one ulp outside)
        lo, hi = (to_sampling(np.asarray(v, dtype=float), prior) for v in box)
        box = (lo, hi)
        x = to_sampling(x, prior, box)
        if population is not None:
            population = to_sampling(np.asarray(population, dtype=float).reshape(x.shape[0], o["walkers"], x.shape[1]), prior, box)
    if population is not None:
        init = np.ascontiguousarray(population, dtype=np.float64).reshape(x.shape[0], o["walkers"], x.shape[1])
    else:
        init = np.stack([ensemble_start(x[s], lo, hi, o["walkers"], o["spread"], o["seed"], int(j_of[s])) for s in range(x.shape[0])])
    o["start"] = "DE's final population" if population is not None else "spread %g around the fit" % o["spread"]
    if a.mcmc_post is not None:
        o["probs"] = _mcmc_post_options(a)["probs"]
        o["masses"] = _mcmc_hpd_masses(a)
    sampler = e.ensemble_sample
    if a.mcmc_post is not None:                            # the summaries on the device; the chain comes back only for --mcmc-out
        post = dict(_mcmc_post_options(a), masses=_mcmc_hpd_masses(a))
        sampler = lambda *args, **kw: e.ensemble_posterior(*args, **kw, burn=o["burn"], keep_chain=bool(a.mcmc_out) or a.mcmc_bands is not None, **post)
    common = dict(split_times=split_times, fit_split=split_times is None, n_step=o["n_step"], thin=o["thin"], seed=o["seed"], ids=np.asarray(j_of, dtype=np.uint64))
    if prior is not None:
        common["prior"] = prior
    joint = _mcmc_joint(a, x.shape[1] - (1 if split_times is None else 0))
    if joint is not None:                                  # the regions on the device, over the kept steps behind the burn-in
        common["joint"] = dict(joint, burn=o["burn"])
    extra = {}
    if o["ladder"] is not None:
        ladder = temperature_ladder(T, o["ladder"][1], o["ladder"][0])
        post = None if a.mcmc_post is None else dict(_mcmc_post_options(a), masses=_mcmc_hpd_masses(a), keep_chain=bool(a.mcmc_out) or a.mcmc_bands is not None)
        res = e.tempered_sample(np.ascontiguousarray(np.repeat(init[:, None], ladder.size, axis=1)), np.asarray(r_of, dtype=np.int32), data, box, ladder,
                                swap_every=o["swap_every"], burn=o["burn"], post=post, **common)
        res["ladder"] = ladder
        extra = {k: res[k] for k in ("ladder", "swap_proposed", "swap_accepted", "rung_llh", "logz")}
    else:
        res = sampler(init, np.asarray(r_of, dtype=np.int32), data, box, temperature=T, **common)
    if a.mcmc_out:
        np.savez(a.mcmc_out, chain=res["chain"], chain_llh=res["chain_llh"], accepted=res["accepted"], last=res["last"], last_llh=res["last_llh"],
                 row=np.asarray(r_of), split=np.asarray(split_times) if split_times is not None else np.empty(0), temperature=float(T), **extra,
                 **({} if prior is None else {"prior_" + k: v for k, v in prior.items()}))
    if a.mcmc_bands is not None:
        # the chain is read back (as for --mcmc-out), mapped to natural units, and its kept samples behind the burn-in - every T-th step -
        # go through the engine once more with the rates kept on the device: a group per fit
        from .optimize import from_sampling
        kept = np.ascontiguousarray(res["chain"][:, o["burn"]::(a.mcmc_bands_thin or 1)])
        nat = kept if prior is None else from_sampling(kept, prior)
        S_, n_, W_, N_ = nat.shape
        pts = nat.reshape(S_ * n_ * W_, N_)
        o["bands_m"] = n_ * W_
        if split_times is None:
            res["bands"] = e.trajectory_bands(pts[:, :-1], pts[:, -1], groups=S_, probs=_probs(a.mcmc_bands))
        else:
            res["bands"] = e.trajectory_bands(pts, np.repeat(np.asarray(split_times, dtype=float), n_ * W_), groups=S_, probs=_probs(a.mcmc_bands))
    if a.mcmc_joint_out:
        from .optimize import joint_table
        j = res["joint"]
        edges = {"edges_%d_%d" % (q, ax): np.stack([t[q]["edges"][ax] for t in joint_table(j)]) for q in range(len(j["pairs"])) for ax in (0, 1)}
        np.savez(a.mcmc_joint_out, **{k_: j[k_] for k_ in ("counts", "range", "inside", "mode", "level", "cells", "held", "pairs", "bins", "offsets", "masses")},
                 burn=o["burn"], **edges, **({} if prior is None else {"prior_scale": prior["scale"]}))
    return o, float(T), res


def print_joint(label, o, res, s):
    """The ``joint:`` lines of fit s: one per pair of --mcmc-joint, from the histograms the device reduced.  Sampling units, except for
    a --mcmc-log coordinate: natural units, the image of a region that is highest-density on the log scale - the line says so."""
    from .optimize import joint_table
    j = res["joint"]
    rows = joint_table({k: (v[s] if k in ("counts", "range", "inside", "mode", "level", "cells", "held") else v) for k, v in j.items()}, prior=o.get("prior"))
    name = lambda c: "st" if o.get("fit_split") and c == res["last"].shape[-1] - 1 else str(c)
    pair = lambda v: "[%r, %r] x [%r, %r]" % (v[0][0], v[0][1], v[1][0], v[1][1])
    for t in rows:
        log = t.get("natural_is_image", False)
        print("joint:", label, "\tcoordinates (%s, %s)" % (name(t["pair"][0]), name(t["pair"][1])), "\tbins = %d x %d" % (len(t["edges"][0]) - 1, len(t["edges"][1]) - 1),
              "\twindow =", pair(t.get("window_natural", t["window"])), "\tinside = %d" % t["inside"],
              "\tmode = (%r, %r)" % tuple(t.get("mode_centre_natural", t["mode_centre"])),
              *("\tmass %g: level = %d cells = %d held = %d / %d extent = %s" % (r["mass"], r["level"], r["cells"], r["held"], t["inside"], pair(r.get("extent_natural", r["extent"])))
                for r in t["regions"]),
              *(["\t(log scale: the region is highest-density in the logarithm; window, mode and extent are its image in natural units)"] if log else []))


def _mcmc_post_options(a):
    """The options of --mcmc-post, or their defaults: the quantiles 0.025 0.5 0.975, every lag."""
    return dict(probs=tuple(a.mcmc_post) if a.mcmc_post else (0.025, 0.5, 0.975), max_lag=a.mcmc_lag)


def _mcmc_hpd_masses(a):
    """The masses of --mcmc-hpd: None without the option, 0.95 where it names none."""
    if a.mcmc_hpd is None:
        return None
    return tuple(a.mcmc_hpd) if a.mcmc_hpd else (0.95,)


def print_post(label, o, res, s):
    """The ``post:`` lines of fit s: one per coordinate, from the summaries the device reduced (Engine.ensemble_posterior)."""
    from .optimize import posterior_table
    n = o["n_step"] // o["thin"] - o["burn"]
    t = posterior_table({k: res[k][s] for k in ("mean", "cov", "quant", "tau", "window", "last", "best_x", "hpd") if k in res}, n, prior=o.get("prior"))
    probs, masses = o["probs"], o.get("masses") or ()
    quant, best_x, hpd = t.get("quant_natural", t["quant"]), t.get("best_x_natural", res["best_x"][s]), t.get("hpd_natural", t.get("hpd"))
    for c in range(res["mean"].shape[1]):
        print("post:", label, "\tcoordinate %d" % c, "\tmean =", t["mean"][c], "\tsd =", t["sd"][c],
              *("\tq%g = %r" % (p, float(quant[c][i])) for i, p in enumerate(probs)),
              *("\thpd %g = [%r, %r]" % (p, float(hpd[c][i][0]), float(hpd[c][i][1])) for i, p in enumerate(masses)), "\ttau =", t["tau"][c], "\tn_eff =", t["n_eff"][c],
              *(["\t(short)"] if t["short"][c] else []), "\tcorr = [" + ", ".join(repr(float(v)) for v in t["corr"][c]) + "]",
              "\tbest llh =", res["best_llh"][s], "at = (%d, %d)" % tuple(res["best_at"][s]), "x =", best_x[c], *_log_note(o, c),
              *(["\t(hpd: the shortest interval of the logarithm, its ends in natural units)"] if masses and _log_note(o, c) else []))


def _log_note(o, c):
    """What a summary line of coordinate c ends on where the coordinate was sampled on the log scale (--mcmc-log)."""
    prior = o.get("prior")
    return ["\t(log scale: quantiles and best sample in natural units, mean, sd and corr of the logarithm)"] if prior is not None and prior["scale"][c] else []


def print_ladder(label, res, s):
    """The ``ladder:`` line of fit s of a tempered run: the temperatures, the swap acceptance per pair (nan: no pair had two values),
    the mean llh per rung and logz."""
    with np.errstate(all="ignore"):
        rate = res["swap_accepted"][s] / res["swap_proposed"][s].astype(float)
    fmt = lambda v: "[" + ", ".join(repr(float(t)) for t in v) + "]"
    print("ladder:", label, "\tT =", fmt(res["ladder"]), "\tswaps accepted =", fmt(rate), "\trung llh =", fmt(res["rung_llh"][s]), "\tlogz =", repr(float(res["logz"][s])))


def print_mcmc(label, o, res, s):
    """The ``mcmc:`` lines of fit s: one per coordinate, from ensemble_summary of its chain - or, with --mcmc-post, its ``post:`` lines;
    of a tempered run (--mcmc-ladder) the cold rung's, and behind them the fit's ``ladder:`` line."""
    if "joint" in res:                                     # behind everything else of the fit
        print_mcmc(label, o, {k: v for k, v in res.items() if k != "joint"}, s)
        return print_joint(label, o, res, s)
    if "logz" in res:
        cold = {k: v for k, v in res.items() if k not in ("logz", "accepted")}
        print_mcmc(label, o, dict(cold, accepted=res["accepted"][:, 0]), s)
        return print_ladder(label, res, s)
    if "quant" in res:
        return print_post(label, o, res, s)
    from .optimize import ensemble_summary
    m = ensemble_summary(res["chain"][s], o["burn"], accepted=res["accepted"][s], n_step=o["n_step"])
    if o.get("prior") is not None:                         # quantiles are monotone under exp: natural units for the log-scale coordinates
        from .optimize import from_sampling
        m.update({k: from_sampling(m[k], o["prior"]) for k in ("median", "q025", "q975")})
    for c in range(res["chain"].shape[3]):
        print("mcmc:", label, "\tcoordinate %d" % c, "\tmean =", m["mean"][c], "\tmedian =", m["median"][c], "\t2.5% =", m["q025"][c], "\t97.5% =", m["q975"][c],
              "\ttau =", m["tau"][c], "\taccepted =", m["acceptance"], *(["\t(short)"] if m["short"][c] else []), *_log_note(o, c))


def print_mcmc_bands(label, mc, s, inp):
    """The `bands:` lines of fit s of --mcmc-bands, behind its other lines."""
    if mc and "bands" in mc[2]:
        for line in bands_lines(label, {k: v[s] for k, v in mc[2]["bands"].items() if k != "probs"}, inp.times, inp.scaleTime, mc[0]["bands_m"]):
            print(line)


def _prior_text(o):
    """The sampler's prior in words, behind _mcmc_text; nothing without --mcmc-log / --mcmc-prior."""
    p = o.get("prior")
    if p is None:
        return ""
    parts = ["coordinate %d %s%s" % (c, "on the log scale" if p["scale"][c] else "linear",
                                     ", normal(%r, %r)" % (float(p["p0"][c]), float(p["p1"][c])) if p["kind"][c] == 1 else
                                     ", exponential(%r)" % float(p["p0"][c]) if p["kind"][c] == 2 else ", flat") for c in range(len(p["scale"]))]
    return "; prior on the sampling coordinates (not tempered): " + "; ".join(parts)


def _mcmc_text(o, T, res, dt):
    return _mcmc_text_(o, T, res, dt) + _prior_text(o)


def _mcmc_text_(o, T, res, dt):
    if o["ladder"] is not None:
        return "tempered ensemble MCMC with %d rungs up to %r x the temperature, a swap round every %d steps, %d walkers per rung, %d steps, thin %d, burn %d, from %s, temperature %r, seed %d: %d ladders in one call, %.3f s, %d proposals evaluated" % (
            o["ladder"][0], o["ladder"][1], o["swap_every"], o["walkers"], o["n_step"], o["thin"], o["burn"], o["start"], T, o["seed"], res["last"].shape[0], dt, res["n_points"])
    return "ensemble MCMC with %d walkers, %d steps, thin %d, burn %d, from %s, temperature %r, seed %d: %d ensembles in one call, %.3f s, %d proposals evaluated" % (
        o["walkers"], o["n_step"], o["thin"], o["burn"], o["start"], T, o["seed"], res["last"].shape[0], dt, res["n_points"])


def _de_options(a):
    """The options of --de, or their defaults: F in [0.5, 1], CR 0.7, seed 0."""
    return dict(pop=a.de[0], maxiter=a.de[1], F=tuple(a.de_F) if a.de_F is not None else (0.5, 1.0), CR=0.7 if a.de_CR is None else a.de_CR,
                seed=0 if a.de_seed is None else a.de_seed, polish=a.de_polish)


def _de_text(o):
    return "differential evolution with %d members, at most %d generations, F in [%g, %g], CR %g, seed %d%s" % (
        o["pop"], o["maxiter"], o["F"][0], o["F"][1], o["CR"], o["seed"], ", polished" if o["polish"] else "")


def _hop_step_seed(a):
    """--hop-step and --hop-seed, or their defaults: SciPy's step size 0.5, seed 0."""
    return (0.5 if a.hop_step is None else a.hop_step), (0 if a.hop_seed is None else a.hop_seed)


def _hops_text(res, *at):
    """What follows a result line under --hops: the accepted hops and the failed minimisations of the search it reports."""
    return " \thops accepted = %d \tfailed minimisations = %d" % (int(res["accepted"][at]), int(res["failures"][at]))


def box_error(a):
    """Why ``--box`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if not a.box:
        return None
    if not (a.grid_solve or a.fit_st or a.polish):
        return "--box constrains the searches of --grid-solve, --fit-st or --polish: give one of them"
    if a.sweep or a.sweep_pu:
        return "--box constrains the searches of ONE model: --sweep / --sweep-pu are not offered with it"
    k = sum(1 for el in a.mi if int(el[4])) + sum(1 for el in a.pu if int(el[3]))
    seen = set()
    for name, lo, hi in a.box:
        if name == "st":
            if not a.fit_st:
                return "--box st bounds the FITTED split: it needs --fit-st (--grid-st scans the splits it is given)"
        elif not name.isdigit() or int(name) >= k:
            return "--box %s: no such coordinate - K is the index of an optimised parameter (0 ... %d here) or st" % (name, k - 1)
        if name in seen:
            return "--box %s is given twice" % name
        seen.add(name)
        try:
            lo, hi = float(lo), float(hi)
        except ValueError:
            return "--box %s %s %s: LO and HI are numbers (inf and -inf are accepted)" % (name, lo, hi)
        if lo != lo or hi != hi:
            return "--box %s: a bound is NaN" % name
        if lo > hi:
            return "--box %s: the lower bound %g is greater than the upper bound %g" % (name, lo, hi)
    return None


def _box(a, k):
    """The ``(lo, hi)`` of the --box options over the k optimised parameters - and, under --fit-st, the split as one coordinate more -
    or None without a --box; a coordinate that no --box names is unbounded."""
    if not a.box:
        return None
    N = k + (1 if a.fit_st else 0)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    for name, l, h in a.box:
        i = k if name == "st" else int(name)
        lo[i], hi[i] = float(l), float(h)
    return lo, hi


def _box_text(a):
    return "box: " + ", ".join("%s in [%g, %g]" % (name, float(l), float(h)) for name, l, h in a.box)


def top_error(a):
    """Why ``--top`` / ``--polish`` cannot run with these options (checked before any file is read or the GPU is touched), or None."""
    if a.top is None and not a.polish:
        return None
    if a.top is None:
        return "--polish polishes the candidates --top K lists: give --top K"
    if not 1 <= a.top <= 8:
        return "--top K keeps at most 8 candidates per row: K must be 1 ... 8 (got %d)" % a.top
    if a.sweep or a.sweep_pu:
        return "--top reduces the grid of --grid-st / --grid-mi: --sweep / --sweep-pu are not offered with it"
    if a.fit_st:
        return "--top lists scanned candidates, --fit-st fits the split time: give one of them"
    if a.grid_solve:
        return "--top lists scanned candidates (--polish searches from them), --grid-solve searches from every pair: give one of them"
    if not (a.grid_st or a.grid_mi):
        return "--top applies to grid mode: it needs --grid-st and/or --grid-mi"
    if a.gpus > 1 or a.devices:
        return "--top runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    if a.polish and not any(int(el[4]) for el in a.mi) and not any(int(el[3]) for el in a.pu):
        return "--polish needs at least one optimised parameter (-mi ... 1 or -pu ... 1)"
    return None


def profile_error(a):
    """Why ``--profile`` / ``--profile-drop`` cannot run with these options (checked before any file is read or the GPU is touched), or
    None."""
    if a.profile is None:
        if a.profile_drop is not None:
            return "--profile-drop sets the support interval of a profile: give --profile AXIS"
        return None
    if len(a.profile) > 2:
        return "--profile takes one axis (a curve) or two axes (a surface): at most two, got %d" % len(a.profile)
    scanned = {int(g[0]) for g in a.grid_mi if g[0].isdigit()}     # (a malformed --grid-mi is for grid mode to refuse, not for this check)
    for axis in a.profile:
        if axis == "st":
            if not a.grid_st:
                return "--profile st: the split time is not scanned - give --grid-st A B [STEP]"
        elif axis.isdigit():
            if int(axis) not in scanned:
                return "--profile %s: parameter %s is not scanned - give --grid-mi %s LO HI N" % (axis, axis, axis)
        else:
            return "--profile %s: unknown axis - an axis is st or the index K of an optimised parameter (--grid-mi K)" % axis
    if len(set(a.profile)) != len(a.profile):
        return "--profile %s %s names the same axis twice" % tuple(a.profile)
    if a.profile_drop is not None and not a.profile_drop >= 0:
        return "--profile-drop must not be negative (got %g)" % a.profile_drop
    if a.top is not None or a.polish:
        return "--profile keeps the best candidate per axis value, --top / --polish the best per row: give one of them"
    if a.fit_st:
        return "--profile reduces a scanned grid, --fit-st fits the split time: give one of them"
    if a.grid_solve:
        return "--profile reduces a scanned grid, --grid-solve searches from every pair: give one of them"
    if a.sweep or a.sweep_pu:
        return "--profile reduces the grid of --grid-st / --grid-mi: --sweep / --sweep-pu are not offered with it"
    if a.gpus > 1 or a.devices:
        return "--profile runs on one GPU (--device); --gpus N > 1 and --devices are not offered with it"
    return None


def result_line(bs_id, split, times, scale_time, mi, x, llh):
    """The result line of one fitted model, exactly as MiSTI.py:240 prints it (what the test.bs scripts grep): ``times`` is the
    interval grid after a fractional split has been inserted (MigrationInference.__init__ extends it in place)."""
    fixed = [float(el[3]) for el in mi if int(el[4]) == 0]
    fixed_s = "fixed = [" + ", ".join(str(v) for v in fixed) + "]" if fixed else ""
    opt_s = "optim = [" + ", ".join(str(v) for v in x) + "]" if len(x) > 0 else ""
    mig_s = fixed_s + "\t" + opt_s if fixed_s and opt_s else fixed_s + opt_s
    return " ".join(str(v) for v in ("bs_id =", bs_id, "\tsplitT =", split, "\ttime =", sum(times[0:ceil(split)]) * scale_time,
                                     "\tmigration rates", mig_s, "\tllh =", llh))


def split_grid_times(times, split):
    """The interval lengths as MigrationInference.__init__ leaves them for ``split`` (MigrationInference.py:89-99): a fractional
    split cuts its interval in two."""
    times = list(times)
    frac = split % 1
    s = int(split)
    if frac != 0.0 and s < len(times):              # (a split beyond the grid has no model: its pairs carry llh = -inf)
        t1 = frac * times[s]
        t2 = times[s] - t1
        times[s] = t1
        times.insert(s + 1, t2)
    return times


def _evaluator(a, inp, bands, pulses, k, device):
    """The batch evaluator of grid mode: ``evaluate(split, params, rows)`` -> an object with ``llk[n][R]`` and ``status[n]``, and a
    function closing it: the HIP engine on ``device``, or on the device list of ``--devices`` (the multi-device C ABI).  There is no
    other evaluator: without a usable GPU the constructor fails."""
    flags = dict(cpfit=a.cpfit, true_eps=a.trueEPS, smooth=not a.nosmooth, unfolded=a.uf)
    if a.devices:
        from .engine import MultiEngine
        e = MultiEngine(inp.times, inp.lambdas, bands, pulses, n_param=k, sample_date=inp.sampleDateDiscr, mixture_th=a.mth,
                        devices=[int(d) for d in a.devices.split(",")], **flags)
    else:
        e = Engine(inp.times, inp.lambdas, bands, pulses, n_param=k, sample_date=inp.sampleDateDiscr, mixture_th=a.mth, device=device, **flags)
    return e.evaluate, e.close


def grid_model(a):
    """What grid mode and --grid-solve share: the split values, the band and pulse records (bands ending at the given split time
    follow each candidate's split under --grid-st), the number of optimised parameters, and one axis per parameter (its -mi/-pu
    initial value, or its --grid-mi mesh)."""
    st0 = a.st
    splits = [st0]
    if a.grid_st:
        lo, hi = a.grid_st[0], a.grid_st[1]
        step = a.grid_st[2] if len(a.grid_st) > 2 else 1.0
        splits = list(np.arange(lo, hi + 0.5 * step, step))
    bands, pulses, k = [], [], 0
    init = []
    for el in a.mi:
        pop, start, end, val, opt = int(el[0]) - 1, int(el[1]), int(el[2]), float(el[3]), int(el[4])
        if a.grid_st and end == int(ceil(st0)):
            end = -1                                  # follows the candidate's split (test.bs/san_sar.bs.sh:36)
        bands.append((pop, start, end, val, k if opt else -1))
        if opt:
            init.append(val)
            k += 1
    for el in a.pu:
        pop, t, val, opt = int(el[0]) - 1, int(el[1]), float(el[2]), int(el[3])
        pulses.append((pop, t, val, k if opt else -1))
        if opt:
            init.append(val)
            k += 1
    axes = [np.array([v]) for v in init]
    for g in a.grid_mi:
        axes[int(g[0])] = np.logspace(np.log10(float(g[1])), np.log10(float(g[2])), int(g[3]))
    return splits, bands, pulses, k, axes


def grid_mode(a, inp, rows):
    """Batched sweep: one Engine, candidates = split values x parameter grid, replicates = JSFS rows."""
    splits, bands, pulses, k, axes = grid_model(a)
    mesh = np.meshgrid(np.array(splits), *axes, indexing="ij")
    split = mesh[0].ravel()
    params = np.stack([m.ravel() for m in mesh[1:]], axis=1) if k else None
    data = np.array(rows if a.all_bs else [rows[a.bsMode] if a.bsMode >= 0 else np.sum(rows, axis=0)], dtype=float)
    # --gpus N: this process is one of N ranks (main() started them); whole chains per rank, one all_gather, rank 0 prints
    from . import dist as mdist
    rank, local, world = mdist.init_from_env()
    t0 = time.time()
    evaluate, close = _evaluator(a, inp, bands, pulses, k, local if world > 1 else a.device)
    try:
        if world > 1:
            llk, status = mdist.evaluate_sharded(evaluate, split, params, data, by_chain=True, with_status=True)
            res = BatchResult(llk.cpu().numpy(), None, status.cpu().numpy())
        else:
            res = evaluate(split, params, data)
    finally:
        close()
    dt = time.time() - t0
    if "WORLD_SIZE" in os.environ:                    # started as a rank (by --gpus N, or by torchrun directly): leave the group in order
        import torch.distributed as tdist
        if tdist.is_initialized():
            tdist.barrier()
            tdist.destroy_process_group()
    if world > 1:
        if rank != 0:
            return 0
        print("Sharded over %d ranks (whole chains per rank; one all_gather of %d x %d log-likelihoods)" % (world, len(split), data.shape[0]))
    for c in range(len(split)):
        pstr = "" if params is None else "\t".join("%.6g" % v for v in params[c])
        for r in range(data.shape[0]):
            print("bs_id =", r if a.all_bs else a.bsMode, "\tsplitT =", split[c], "\tparams", pstr, "\tllh =", res.llk[c, r],
                  "\tstatus =", int(res.status[c]))
    best = np.unravel_index(np.argmax(np.where(np.isfinite(res.llk), res.llk, -np.inf)), res.llk.shape)
    print("\nbest: splitT =", split[best[0]], "params =", None if params is None else list(params[best[0]]),
          "replicate =", best[1], "llh =", res.llk[best])
    if a.all_bs and len(splits) > 1 and data.shape[0] > 1:
        # the bootstrap confidence interval of test.bs/bs_conf_int.ipynb: per replicate the split of the best candidate,
        # then a Student-t interval of those maxima (row 0 of a -bs file is the sum of the chunks, as there)
        from .optimize import bootstrap_split_interval
        mean, (lo, hi), best_split = bootstrap_split_interval(res.llk, split)
        print("bootstrap: best splitT per replicate mean = %.6g, 95%% interval = [%.6g, %.6g] over %d replicates"
              % (mean, lo, hi, data.shape[0]))
    print("Evaluated %d candidates x %d replicates in %.3f s (%.0f llk evals/s); %.1f%% without a value"
          % (len(split), data.shape[0], dt, res.llk.size / dt, 100 * res.fraction_failed))
    return 0


def grid_top(a, inp, rows):
    """Grid mode with --top K: the same candidates and rows, evaluated without replicates and reduced on the device to the K best
    candidates per row (optimize.scan_best); with --polish one batched search from those (optimize.scan_polish)."""
    from .optimize import _t_interval, scan_best, scan_polish
    splits, bands, pulses, k, axes = grid_model(a)
    mesh = np.meshgrid(np.array(splits), *axes, indexing="ij")
    split = mesh[0].ravel()
    params = np.stack([m.ravel() for m in mesh[1:]], axis=1) if k else None
    data, ids = _data_rows(a, rows)
    flags = dict(cpfit=a.cpfit, true_eps=a.trueEPS, smooth=not a.nosmooth, unfolded=a.uf)
    t0 = time.time()
    with Engine(inp.times, inp.lambdas, bands, pulses, n_param=k, sample_date=inp.sampleDateDiscr, mixture_th=a.mth, device=a.device, **flags) as e:
        if a.polish:
            pol = scan_polish(e, split, params, data, a.top, tol=a.tol, maxiter=1000, box=_box(a, k))
            best, best_llk, status = pol["best"], pol["best_llk"], pol["scan_status"]
        else:
            best, best_llk, status = scan_best(e, split, params, data, a.top)
    dt = time.time() - t0
    R = data.shape[0]
    for r in range(R):
        for j in range(a.top):
            c = best[r, j]
            if c < 0:
                continue
            pstr = "" if params is None else "\t".join("%.6g" % v for v in params[c])
            print("bs_id =", ids[r], "\tsplitT =", split[c], "\tparams", pstr, "\tllh =", best_llk[r, j], "\tstatus =", int(status[c]))
    has = best[:, 0] >= 0
    if has.any():
        # grid mode's best: the first maximum of the table in candidate-major order - the lowest candidate, then the lowest row
        top = best_llk[:, 0].max()
        c, r = min((best[r, 0], r) for r in range(R) if has[r] and best_llk[r, 0] == top)
        print("\nbest: splitT =", split[c], "params =", None if params is None else list(params[c]), "replicate =", r, "llh =", best_llk[r, 0])
    else:
        print("\nbest: no candidate has a value")
    if a.all_bs and len(splits) > 1 and R > 1:
        # grid mode's interval (test.bs/bs_conf_int.ipynb) from the rows' first places; a row without a value counts as candidate 0, as there
        mean, (lo, hi), _ = _t_interval(split[np.where(has, best[:, 0], 0)], 0.95)
        print("bootstrap: best splitT per replicate mean = %.6g, 95%% interval = [%.6g, %.6g] over %d replicates" % (mean, lo, hi, R))
    if a.polish:
        print()
        for r in range(R):
            if not np.isfinite(pol["llh"][r]):
                print("polish: bs_id =", ids[r], "has no finite llh from any listed candidate")
                continue
            st = float(pol["split"][r])
            print(result_line(ids[r], st, split_grid_times(inp.times, st), inp.scaleTime, a.mi, pol["x"][r], pol["llh"][r]))
        if a.box:
            print("polish:", _box_text(a))
        print("polish: %d searches in one batched search (%d rows x at most %d listed candidates); %d rows ended on the iteration cap"
              % (pol["searches"]["cand"].size, R, a.top, int((pol["status"] == 2).sum())))
    print("Evaluated %d candidates x %d replicates in %.3f s (%.0f llk evals/s); %.1f%% without a value"
          % (len(split), R, dt, len(split) * R / dt, 100 * float((status != 0).mean())))
    return 0


def grid_profile(a, inp, rows):
    """Grid mode with --profile: the same candidates and rows, evaluated without replicates and reduced on the device to the best
    candidate per row and per value of the named axis or pair of axes (optimize.scan_profile; the labels are optimize.axis_groups of
    the grid's shape: the split is its outermost axis, parameter K its axis 1 + K)."""
    from .optimize import _t_interval, axis_groups, profile_interval, scan_profile
    splits, bands, pulses, k, axes = grid_model(a)
    mesh = np.meshgrid(np.array(splits), *axes, indexing="ij")
    split = mesh[0].ravel()
    params = np.stack([m.ravel() for m in mesh[1:]], axis=1) if k else None
    data, ids = _data_rows(a, rows)
    which = [0 if t == "st" else 1 + int(t) for t in a.profile]
    names = ["st" if t == "st" else "p" + t for t in a.profile]
    values = [np.asarray(mesh[w]).ravel() for w in which]                 # per candidate: its value on each named axis
    group, G = axis_groups(mesh[0].shape, which)
    flags = dict(cpfit=a.cpfit, true_eps=a.trueEPS, smooth=not a.nosmooth, unfolded=a.uf)
    t0 = time.time()
    with Engine(inp.times, inp.lambdas, bands, pulses, n_param=k, sample_date=inp.sampleDateDiscr, mixture_th=a.mth, device=a.device, **flags) as e:
        prof, best, status = scan_profile(e, split, params, data, group, G)
    dt = time.time() - t0
    R = data.shape[0]
    at = np.full(G, -1, dtype=np.int64)                                   # any member of each group: it carries the group's axis values
    at[group] = np.arange(group.size)
    text = lambda t, v: str(v) if t == "st" else "%.6g" % v
    for r in range(R):
        for g in range(G):
            where = " \t".join("%s = %s" % (nm, text(t, v[at[g]])) for nm, t, v in zip(names, a.profile, values))
            c = best[r, g]
            if c < 0:                                                     # (the group has no value: llh = -inf and no candidate)
                print("bs_id =", ids[r], "\tprofile", where, "\tllh =", prof[r, g])
                continue
            pstr = "" if params is None else "\t".join("%.6g" % v for v in params[c])
            print("bs_id =", ids[r], "\tprofile", where, "\tllh =", prof[r, g], "\tsplitT =", split[c], "\tparams", pstr, "\tstatus =", int(status[c]))
    has = (best >= 0).any(axis=1)
    # per row the lowest candidate that attains the row's maximum: the table's first maximum of that row
    top = prof.max(axis=1)
    first = np.array([best[r][prof[r] == top[r]].min() if has[r] else -1 for r in range(R)], dtype=np.int64)
    if has.any():
        # grid mode's best: the first maximum of the table in candidate-major order - the lowest candidate, then the lowest row
        c, r = min((first[r], r) for r in range(R) if top[r] == top.max())
        print("\nbest: splitT =", split[c], "params =", None if params is None else list(params[c]), "replicate =", r, "llh =", top[r])
    else:
        print("\nbest: no candidate has a value")                       # (as --top prints it; grid mode names candidate 0 with llh = -inf there)
    if len(a.profile) == 1:
        drop = a.profile_drop
        if drop is None:
            from scipy import stats
            drop = 0.5 * stats.chi2.ppf(0.95, 1)
        axis_values = np.asarray(splits if a.profile[0] == "st" else axes[int(a.profile[0])], dtype=float)
        iv = profile_interval(prof, axis_values, drop)
        for r in range(R):
            if not has[r]:
                print("support: bs_id =", ids[r], "has no value at any %s" % names[0])
                continue
            print("support: bs_id =", ids[r], "best %s =" % names[0], text(a.profile[0], iv["best"][r]), "llh =", iv["llh"][r],
                  "within %.6g of it: %s in [%s, %s]" % (drop, names[0], text(a.profile[0], iv["lo"][r]), text(a.profile[0], iv["hi"][r])))
    if a.all_bs and "st" in a.profile and len(splits) > 1 and R > 1:
        # grid mode's interval (test.bs/bs_conf_int.ipynb) from the rows' arg-max; a row without a value counts as candidate 0, as there
        mean, (lo, hi), _ = _t_interval(split[np.where(has, first, 0)], 0.95)
        print("bootstrap: best splitT per replicate mean = %.6g, 95%% interval = [%.6g, %.6g] over %d replicates" % (mean, lo, hi, R))
    print("Evaluated %d candidates x %d replicates in %.3f s (%.0f llk evals/s); %.1f%% without a value"
          % (len(split), R, dt, len(split) * R / dt, 100 * float((status != 0).mean())))
    return 0


def grid_solve(a, inp, rows):
    """The bootstrap profiles of the reference's test.bs scripts (``for bs in 0..B; for st in A..Z: MiSTI.py ... ${st} -bs ${bs}
    -mi ...``, one Solve per pair) as ONE batched search: every (row, split, start) triple is a start of misti_nm_solve_rows."""
    from .optimize import bootstrap_profile, bootstrap_profile_de, bootstrap_profile_global, bootstrap_profile_interval
    splits, bands, pulses, k, axes = grid_model(a)
    starts = np.stack([m.ravel() for m in np.meshgrid(*axes, indexing="ij")], axis=1)
    data = np.array(rows if a.all_bs else [rows[a.bsMode] if a.bsMode >= 0 else np.sum(rows, axis=0)], dtype=float)
    ids = list(range(data.shape[0])) if a.all_bs else [a.bsMode]
    flags = dict(cpfit=a.cpfit, true_eps=a.trueEPS, smooth=not a.nosmooth, unfolded=a.uf)
    hop_step, hop_seed = _hop_step_seed(a)
    t0 = time.time()
    with Engine(inp.times, inp.lambdas, bands, pulses, n_param=k, sample_date=inp.sampleDateDiscr, mixture_th=a.mth, device=a.device, **flags) as e:
        if a.de:
            prof = bootstrap_profile_de(e, splits, data, starts[0], _box(a, k), polish_tol=a.tol, return_population=_mcmc_from_de(a), **_de_options(a))
        elif a.hops:
            prof = bootstrap_profile_global(e, splits, data, starts, seed=hop_seed, niter=a.hops, T=0.5, stepsize=hop_step, box=_box(a, k))
        else:
            prof = bootstrap_profile(e, splits, data, starts, tol=a.tol, maxiter=1000, box=_box(a, k))
        if a.se:
            # one stencil per printed fit, all of them in one call: row outermost, split innermost, as the lines
            R_, P_ = data.shape[0], len(splits)
            cur = e.curvature(prof["x"].reshape(R_ * P_, k), np.tile(np.asarray(splits, dtype=float), R_), np.repeat(np.arange(R_), P_), data,
                              rel_step=_se_step(a))
        bands_text = None
        if a.bands is not None:
            # every row at its own best split (a row without a finite llh at any split: no sample)
            has_ = np.isfinite(prof["llh"]).any(axis=1)
            at_ = np.argmax(np.where(np.isfinite(prof["llh"]), prof["llh"], -np.inf), axis=1)
            bands_text = _captured(run_bands, a, e, np.where(has_[:, None], prof["x"][np.arange(data.shape[0]), at_], np.nan),
                                   np.where(has_, np.asarray(splits, dtype=float)[at_], np.nan), inp)
        mc, dt_mc = None, 0.0
        if a.mcmc:
            # one ensemble per printed fit: row outermost, split innermost, as the lines; the stream of a fit is its split's index
            t1 = time.time()
            R_, P_ = data.shape[0], len(splits)
            mc = run_mcmc(a, e, prof["x"].reshape(R_ * P_, k), np.repeat(np.arange(R_), P_), np.tile(np.arange(P_), R_), data, _box(a, k),
                          np.tile(np.asarray(splits, dtype=float), R_), a.uf, prof["population"] if _mcmc_from_de(a) else None)
            if isinstance(mc, str):
                print(mc, file=sys.stderr)
                return 2
            dt_mc = time.time() - t1
    dt = time.time() - t0 - dt_mc
    for r in range(data.shape[0]):
        for p, st in enumerate(splits):
            print(result_line(ids[r], st, split_grid_times(inp.times, st), inp.scaleTime, a.mi, prof["x"][r, p], prof["llh"][r, p])
                  + (_hops_text(prof, r, p) if a.hops else ""))
            if mc:
                print_mcmc("bs_id = %s \tsplitT = %s" % (ids[r], st), mc[0], mc[2], r * len(splits) + p)
                print_mcmc_bands("bs_id = %s \tsplitT = %s" % (ids[r], st), mc, r * len(splits) + p, inp)
    if a.se:
        print()
        print_se(["bs_id = %s \tsplitT = %s" % (ids[r], st) for r in range(data.shape[0]) for st in splits], cur,
                 data if a.all_bs and data.shape[0] >= 4 else None, a.uf)
    iv = bootstrap_profile_interval(prof["llh"], splits, prof["x"])
    print()
    if bands_text:
        print(bands_text)
    if iv["data_split"] is None:
        print("grid-solve: bs_id =", ids[0], "has no finite llh at any split")
    else:
        print("grid-solve: bs_id =", ids[0], "best splitT =", iv["data_split"], "optim = [" + ", ".join(str(v) for v in iv["data_x"]) + "]",
              "llh =", iv["data_llh"])
    if a.jackknife is not None:
        # every rate at the row's own best split (NaN for a row without a finite llh at any split)
        has = np.isfinite(prof["llh"]).any(axis=1)
        at = np.argmax(np.where(np.isfinite(prof["llh"]), prof["llh"], -np.inf), axis=1)
        theta = np.where(has[:, None], prof["x"][np.arange(data.shape[0]), at], np.nan)
        print_jackknife(["optim[%d]" % i for i in range(k)], theta, data[:, 0])
    elif iv["interval"] is None:
        print("grid-solve: no bootstrap interval (%d bootstrap rows with a best split; at least 2 needed)" % iv["n_boot"])
    else:
        print("grid-solve: bootstrap best splitT mean =", iv["mean"], "97.5%% t-interval = [%r, %r]" % tuple(float(v) for v in iv["interval"]),
              "over %d replicates (%d without a value excluded)" % (iv["n_boot"], iv["n_excluded"]))
    n = prof["llh"].size
    if a.box:
        print("grid-solve:", _box_text(a))
    if mc:
        print("grid-solve:", _mcmc_text(mc[0], mc[1], mc[2], dt_mc))
    if a.de:
        print("grid-solve:", _de_text(_de_options(a)))
        print("grid-solve: %d pairs in one population search, %.3f s, %d points; %d pairs ended on the generation cap, %d without a value"
              % (n, dt, prof["n_points"], int((prof["status"] == 2).sum()), int((~np.isfinite(prof["llh"])).sum())))
        return 0
    if a.hops:
        print("grid-solve: basin hopping with %d hops, step %g, seed %d" % (a.hops, hop_step, hop_seed))
        print("grid-solve: %d pairs x %d starts in one global search, %.3f s; %d pairs with a failed minimisation, %d without a value"
              % (n, starts.shape[0], dt, int((prof["failures"] > 0).sum()), int((~np.isfinite(prof["llh"])).sum())))
        return 0
    print("grid-solve: %d pairs x %d starts in one search, %.3f s; %d pairs ended on the iteration cap, %d without a value"
          % (n, starts.shape[0], dt, int((prof["status"] == 2).sum()), int((~np.isfinite(prof["llh"])).sum())))
    return 0


def fit_st(a, inp, rows):
    """--fit-st: the split time as a coordinate - per JSFS row one search over (optimised parameters, split) from every (start,
    initial split) pair, all in ONE misti_nm_solve_split call; the best search per row is printed."""
    from .optimize import split_fit, split_fit_de, split_fit_global, split_fit_interval
    splits, bands, pulses, k, axes = grid_model(a)
    starts = np.stack([m.ravel() for m in np.meshgrid(*axes, indexing="ij")], axis=1) if k else np.empty((1, 0))
    data, ids = _data_rows(a, rows)
    flags = dict(cpfit=a.cpfit, true_eps=a.trueEPS, smooth=not a.nosmooth, unfolded=a.uf)
    hop_step, hop_seed = _hop_step_seed(a)
    t0 = time.time()
    with Engine(inp.times, inp.lambdas, bands, pulses, n_param=k, sample_date=inp.sampleDateDiscr, mixture_th=a.mth, device=a.device, **flags) as e:
        if a.de:
            fit = split_fit_de(e, data, np.append(starts[0], splits[0]), _box(a, k), polish_tol=a.tol, return_population=_mcmc_from_de(a), **_de_options(a))
        elif a.hops:
            fit = split_fit_global(e, data, starts, splits, seed=hop_seed, niter=a.hops, T=0.5, stepsize=hop_step, box=_box(a, k))
        else:
            fit = split_fit(e, data, starts, splits, tol=a.tol, maxiter=1000, box=_box(a, k))
        bands_text = None
        if a.bands is not None:
            bands_text = _captured(run_bands, a, e, np.where(np.isfinite(fit["llh"])[:, None], fit["x"][:, :k], np.nan), fit["split"], inp)
        mc, dt_mc = None, 0.0
        if a.mcmc:
            # one ensemble per row over (optimised parameters, split); the rows of a bootstrap share stream 0
            t1 = time.time()
            R_ = data.shape[0]
            mc = run_mcmc(a, e, np.hstack([fit["x"][:, :k], np.asarray(fit["split"], dtype=float)[:, None]]), np.arange(R_), np.zeros(R_, dtype=int),
                          data, _box(a, k), None, a.uf, fit["population"] if _mcmc_from_de(a) else None)
            if isinstance(mc, str):
                print(mc, file=sys.stderr)
                return 2
            dt_mc = time.time() - t1
    dt = time.time() - t0 - dt_mc
    for r in range(data.shape[0]):
        st = float(fit["split"][r])
        if not np.isfinite(fit["llh"][r]):
            print("fit-st: bs_id =", ids[r], "has no finite llh from any start")
            continue
        print(result_line(ids[r], st, split_grid_times(inp.times, st), inp.scaleTime, a.mi, fit["x"][r, :k], fit["llh"][r])
              + (_hops_text(fit, r) if a.hops else ""))
        if mc:
            print_mcmc("bs_id = %s \tsplitT = %s" % (ids[r], st), mc[0], mc[2], r)
            print_mcmc_bands("bs_id = %s \tsplitT = %s" % (ids[r], st), mc, r, inp)
    print()
    if bands_text:
        print(bands_text)
    if a.jackknife is not None:
        has = np.isfinite(fit["llh"]) & np.isfinite(fit["split"])
        theta = np.where(has[:, None], np.hstack([fit["split"][:, None], fit["x"][:, :k]]), np.nan)
        print_jackknife(["splitT"] + ["optim[%d]" % i for i in range(k)], theta, data[:, 0])
    elif a.all_bs:
        iv = split_fit_interval(fit["split"], fit["llh"])
        if iv["interval"] is None:
            print("fit-st: no bootstrap interval (%d bootstrap rows with a fitted split; at least 2 needed)" % iv["n_boot"])
        else:
            print("fit-st: bootstrap fitted splitT mean =", iv["mean"], "95%% t-interval = [%r, %r]" % iv["interval"],
                  "over %d replicates (%d without a value excluded)" % (iv["n_boot"], iv["n_excluded"]))
    if a.box:
        print("fit-st:", _box_text(a))
    if mc:
        print("fit-st:", _mcmc_text(mc[0], mc[1], mc[2], dt_mc))
    if a.de:
        print("fit-st:", _de_text(_de_options(a)))
        print("fit-st: %d rows in one population search, %.3f s, %d points; %d rows ended on the generation cap, %d without a value"
              % (data.shape[0], dt, fit["n_points"], int((fit["status"] == 2).sum()), int((~np.isfinite(fit["llh"])).sum())))
        return 0
    if a.hops:
        print("fit-st: basin hopping with %d hops, step %g, seed %d" % (a.hops, hop_step, hop_seed))
        print("fit-st: %d rows x %d (start, initial split) pairs in one global search, %.3f s; %d rows with a failed minimisation, %d without a value"
              % (data.shape[0], starts.shape[0] * len(splits), dt, int((fit["failures"] > 0).sum()), int((~np.isfinite(fit["llh"])).sum())))
        return 0
    print("fit-st: %d rows x %d (start, initial split) pairs in one search, %.3f s; %d rows ended on the iteration cap, %d without a value"
          % (data.shape[0], starts.shape[0] * len(splits), dt, int((fit["status"] == 2).sum()), int((~np.isfinite(fit["llh"])).sum())))
    return 0


def _sweep_models(a, inp, plan):
    """Which models of the sweep the reference would have run (SetModel's checks; it exits in PrintError for the others), and the
    Engine for them: band and pulse records with the bounds and times of the first of them (every batch passes its own)."""
    from .sweep import structure_error
    pops = [b[0] for b in plan.bands]
    numT = len(inp.lambdas)
    ok = np.array([structure_error(plan.split[m], plan.bounds[m], pops, inp.sampleDateDiscr, numT, plan.pulse_times[m], plan.pulse_values[m])
                   is None for m in range(plan.n_model)], dtype=bool)
    if not ok.any():
        return ok, None
    first = int(np.argmax(ok))
    flags = dict(cpfit=a.cpfit, true_eps=a.trueEPS, smooth=not a.nosmooth, unfolded=a.uf)
    eng = Engine(inp.times, inp.lambdas, plan.engine_bands(first), plan.engine_pulses(first), n_param=plan.n_param, sample_date=inp.sampleDateDiscr,
                 mixture_th=a.mth, device=a.device, **flags)
    return ok, eng


def _data_rows(a, rows):
    """The JSFS rows of a batched run and their bs_id: every row (--all-bs), row -bs N, or the sum of all rows (as the single run)."""
    if a.all_bs:
        return np.array(rows, dtype=float), list(range(len(rows)))
    one = rows[a.bsMode] if a.bsMode >= 0 else [sum(r[i] for r in rows) for i in range(8)]
    return np.array([one], dtype=float), [a.bsMode]


def _model_text(plan, m, names):
    return " ".join("%s = %s" % (n, plan.assign[m][n]) for n in names)


def _print_sweep_interval(plan, ids, llh, x=None):
    """The bs_conf_int.ipynb reduction per swept variable (optimize.sweep_interval) of a printed table llh[R][M]."""
    from .optimize import sweep_interval
    iv = sweep_interval(llh, plan.values, x)
    if iv["data_model"] is None:
        print("sweep: bs_id =", ids[0], "has no finite llh at any model")
    else:
        m = iv["data_model"]
        opt = "" if x is None else " optim = [" + ", ".join(str(v) for v in iv["data_x"]) + "]"
        print("sweep: bs_id =", ids[0], "best model", _model_text(plan, m, plan.model_names) + opt, "llh =", iv["data_llh"])
    for n, v in zip(plan.model_names, iv["variables"]):
        if v["interval"] is None:
            print("sweep: %s: no bootstrap interval (%d bootstrap rows with a best model; at least 2 needed)" % (n, v["n_boot"]))
        else:
            print("sweep: %s bootstrap mean =" % n, v["mean"], "97.5%% t-interval = [%r, %r]" % tuple(float(t) for t in v["interval"]),
                  "over %d replicates (%d without a value excluded)" % (v["n_boot"], v["n_excluded"]))


def sweep_eval(a, inp, rows):
    """The GNU-parallel recipe (README.md:110-115 of the reference) in ONE evaluation: every model of the sweep x every JSFS row,
    per-candidate band bounds; per model the MiSTI.py:240 line the single run prints (rows outermost, then the sweeps in the order
    given), nothing for a model the reference would have exited on."""
    from .sweep import expand
    plan = expand(a)
    data, ids = _data_rows(a, rows)
    t0 = time.time()
    ok, eng = _sweep_models(a, inp, plan)
    M, R = plan.n_model, data.shape[0]
    llh = np.full((R, M), -np.inf)
    status = np.full(M, 4, dtype=np.int32)
    if eng is not None:
        sel = np.where(ok)[0]
        with eng:
            res = eng.evaluate(plan.split[sel], plan.params[sel] if plan.n_param else None, data, band_bounds=plan.bounds[sel],
                               pulse_times=plan.pulse_times[sel] if plan.pulse_swept else None)
        llh[:, sel] = res.llk.T
        status[sel] = res.status
    dt = time.time() - t0
    # no line where the reference exits: SetModel's checks, or an infinite coalescent time (JAFSpectrum's PrintError)
    shown = ok & (status != 3) & (status != 4)
    for r in range(R):
        for m in np.where(shown)[0]:
            print(result_line(ids[r], float(plan.split[m]), split_grid_times(inp.times, plan.split[m]), inp.scaleTime, plan.mi[m],
                              plan.params[m, :plan.k], float(llh[r, m])))
    print()
    table = np.where(shown[None, :], llh, -np.inf)
    if np.isfinite(table).any():
        r, m = np.unravel_index(np.argmax(np.where(np.isfinite(table), table, -np.inf)), table.shape)
        print("sweep: best model", _model_text(plan, m, plan.names), "bs_id =", ids[r], "llh =", float(table[r, m]))
    else:
        print("sweep: no model has a finite llh")
    if a.all_bs and R > 1:
        _print_sweep_interval(plan, ids, table)
    print("sweep: %d models x %d rows in one evaluation, %.3f s; %d models skipped (SetModel's checks or no finite coalescent time)"
          % (M, R, dt, int((~shown).sum())))
    return 0


def sweep_solve(a, inp, rows):
    """--grid-solve with --sweep: the boundary profiles ("when did migration start or stop") as ONE batched search - every
    (row, model, start) triple is a start of misti_nm_solve_bounds (misti_nm_solve_pulses when a pulse time is swept), the best
    start kept per (row, model)."""
    from .optimize import sweep_profile
    from .sweep import expand
    plan = expand(a)
    data, ids = _data_rows(a, rows)
    t0 = time.time()
    ok, eng = _sweep_models(a, inp, plan)
    M, R = plan.n_model, data.shape[0]
    llh = np.full((R, M), -np.inf)
    x = np.full((R, M, plan.k), np.nan)
    status = np.zeros((R, M), dtype=np.int32)
    sel = np.where(ok)[0]
    if eng is not None:
        with eng:
            models = [(plan.split[m], plan.bounds[m]) + ((plan.pulse_times[m],) if plan.pulse_swept else ()) for m in sel]
            prof = sweep_profile(eng, models, data, plan.starts, tol=a.tol, maxiter=1000)
        llh[:, sel], x[:, sel], status[:, sel] = prof["llh"], prof["x"], prof["status"]
    dt = time.time() - t0
    for r in range(R):
        for m in sel:
            print(result_line(ids[r], float(plan.split[m]), split_grid_times(inp.times, plan.split[m]), inp.scaleTime, plan.mi[m], x[r, m],
                              float(llh[r, m])))
    print()
    _print_sweep_interval(plan, ids, llh, x)
    print("sweep: %d (row, model) pairs x %d starts in one search, %.3f s; %d models skipped (SetModel's checks), %d pairs ended on "
          "the iteration cap, %d without a value" % (R * len(sel), plan.starts.shape[0], dt, M - len(sel),
                                                     int((status[:, sel] == 2).sum()), int((~np.isfinite(llh[:, sel])).sum())))
    return 0


def main(argv=None):
    t0 = time.time()
    a = build_parser().parse_args(argv)
    why = jackknife_error(a) or parametric_error(a) or bootstrap_error(a) or se_error(a) or profile_error(a) or top_error(a) or hops_error(a) or de_error(a) or mcmc_error(a) or bands_error(a) or fit_st_error(a) or sweep_error(a) or grid_solve_error(a) or box_error(a)
    if why:
        print(why, file=sys.stderr)
        return 2
    if a.bootstrap is not None or a.parametric is not None or a.jackknife is not None:
        a.all_bs = True                                     # every mode below sees a bootstrap (or jackknife) table
    # the two ways of using several GPUs exclude each other: N ranks that each opened the whole device list would run N x D contexts
    if a.gpus > 1 and a.devices:
        print("--gpus (one rank per GPU) and --devices (a device list in one process) exclude each other", file=sys.stderr)
        return 2
    if a.devices and not (a.grid_st or a.grid_mi or a.all_bs):
        print("--devices applies to the batched sweep (--grid-st / --grid-mi / --all-bs); a single model runs on --device", file=sys.stderr)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if not (a.grid_st or a.grid_mi or a.all_bs):
            print("--gpus applies to the batched sweep (--grid-st / --grid-mi / --all-bs); a single model runs on one GPU", file=sys.stderr)
        else:
            # Start the ranks as CHILD processes and pass rank 0's output through.  This process has not imported torch or touched
            # HIP and never does (a process that has initialised the GPU must not be forked or replaced); the reference's way of
            # using N processors is `parallel -j N ./MiSTI.py ... >> res.out` (/root/reference/README.md:110-115).
            from . import dist as mdist
            code, out = mdist.launch_ranks(a.gpus, list(sys.argv[1:] if argv is None else argv), module=RANK_MODULE)
            sys.stdout.write(out)
            sys.stdout.flush()
            return code
    quiet = int(os.environ.get("RANK", "0")) != 0           # a rank other than 0 of a --gpus run: it computes, rank 0 reports
    if quiet:
        sys.stdout = open(os.devnull, "w")
    units = mio.Units.from_file(a.funits)
    print(units.describe())
    if a.hetloss is not None:
        units.set_hetloss(a.hetloss)
    print(" ".join(sys.argv))
    print(time.strftime("Job run at %H:%M:%S on %d %b %Y"))
    f1, f2, fj = (os.path.join(a.wd, f) for f in (a.fpsmc1, a.fpsmc2, a.fjafs))
    print("Reading from files:")
    print("pop1\t", f1)
    print("pop2\t", f2)
    print("jafs\t", fj)
    rows, pop1, pop2 = mio.read_jsfs(fj)
    if a.bootstrap is not None:
        from .optimize import check_chunks
        try:
            check_chunks(rows)                              # what the ABI would refuse, said before the GPU is touched
        except ValueError as e:
            print("--bootstrap: %s: %s" % (fj, e), file=sys.stderr)
            return 2
    if a.jackknife is not None:
        from .optimize import check_jackknife, jackknife_weights
        try:
            if a.jackknife >= 1:
                check_jackknife(rows, a.jackknife)          # what the ABI would refuse, said before the GPU is touched
            else:
                jackknife_weights([r[0] for r in rows])     # the file is the table: its column 0 must be one's
        except ValueError as e:
            print("--jackknife: %s: %s" % (fj, e), file=sys.stderr)
            return 2
    if a.bsMode == -1:
        inputSFS = [sum(r[i] for r in rows) for i in range(8)]
    else:
        inputSFS = rows[a.bsMode]
    print("IMPORTANT NOTICE!!! Every time you are running MiSTI, make sure that psmc files are supplied in the same "
          "order as populations appear in the joint allele frequency spectrum.")
    fout = os.path.join(a.wd, a.fout) if a.fout else ""
    inp = mio.read_psmc(f1, f2, a.sdate, a.rd, units)
    if a.bootstrap is not None:
        n_chunk = len(rows)
        rows = bootstrap_rows(a, inp, rows, pop1, pop2)
        print("Bootstrap: %d replicates of %d chunks drawn on the device (seed %d%s): the project's own stream, not the reference's"
              % (a.bootstrap, n_chunk, a.bs_seed or 0, ", normalized" if a.bs_normalize else ""))
    if a.jackknife:
        n_chunk = len(rows)
        rows = jackknife_rows(a, inp, rows, pop1, pop2)
        print("Jackknife: %d leave-out rows of %d chunks in groups of %d made on the device" % (len(rows) - 1, n_chunk, a.jackknife))
    if a.parametric is not None:
        rows = parametric_rows(a, inp, inputSFS, pop1, pop2)
        if rows is None:
            print("Failed to fit such a model: --parametric has no spectrum to draw from.")
            return 1
    if a.sweep or a.sweep_pu:
        return sweep_solve(a, inp, rows) if a.grid_solve else sweep_eval(a, inp, rows)
    inp.divergenceTime = a.st
    if a.fit_st:
        return fit_st(a, inp, rows)
    if a.grid_solve:
        return grid_solve(a, inp, rows)
    if a.top is not None:
        return grid_top(a, inp, rows)
    if a.profile is not None:
        return grid_profile(a, inp, rows)
    if a.grid_st or a.grid_mi or a.all_bs:
        return grid_mode(a, inp, rows)

    t1 = time.time()
    mig = MigrationInference(inp.times, inp.lambdas, inputSFS, inp.divergenceTime, a.mi, a.pu,
                             thrh=[inp.theta, inp.rho], Tpsmc=inp.Tpsmc, enableOutput=False, smooth=not a.nosmooth,
                             unfolded=a.uf, trueEPS=a.trueEPS, sampleDate=inp.sampleDateDiscr, mixtureTH=a.mth,
                             cpfit=a.cpfit, device=a.device)
    sol = mig.Solve(a.tol)
    print(sol)
    print("\nParameter estimates:")
    # inp.times was extended in place by a fractional split, as in the reference (MiSTI.py:240)
    print(result_line(a.bsMode, inp.divergenceTime, inp.times, inp.scaleTime, a.mi, sol[0], sol[1]))
    if a.se and sol[1] != -10 ** 9:
        # a -bs N run on a bootstrap table (row 0 the data, resamples behind it) has the rows the sandwich needs; the sum of all rows has not
        boot = np.array(rows, dtype=float) if a.bsMode >= 0 and len(rows) >= 4 else None
        cur = mig._engine.curvature([list(sol[0])], [a.st], [max(a.bsMode, 0)] if boot is not None else [0],
                                    boot if boot is not None else [inputSFS], rel_step=_se_step(a))
        print_se(["bs_id = %s \tsplitT = %s" % (a.bsMode, a.st)], cur, boot, a.uf)
    print("\n")
    t2 = time.time()
    if sol[1] == -10 ** 9:
        print("Failed to fit such a model.")
    elif a.bsMode == 0:
        llh = mig.llh if len(sol[0]) == 0 else mig.JAFSLikelihood(sol[0])
        text = mio.format_migration(mig, llh, inp.scaleTime, inp.scaleEPS)
        if fout == "":
            print(text)
        else:
            with open(fout, "w") as fw:
                fw.write(text)
    MigrationInference.Report()
    print("Runtime:   optimisation", t2 - t1)
    print("           total       ", time.time() - t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
