"""Named sweep variables on the command line: the reference's GNU-parallel recipe (README.md:110-115 of the reference)

    parallel ./MiSTI.py g1.psmc g2.psmc sim.jafs {st} -uf -mi 1 0 {mc} {mi1} 0 -mi 2 0 {mc} {mi2} 0 \\
             -mi 1 {mc} {st} {mi3} 0 -mi 2 {mc} {st} {mi4} 0 >> res.out ::: st 20 .. 25 ::: mc 8 .. 12 ::: mi1 0 0.5 2 5 ...

as ONE command: ``{NAME}`` stands in the positional split time and in the start, end and rate fields of ``-mi``, and
``--sweep NAME V1 V2 ...`` is the recipe's ``::: NAME V1 V2 ...``.  This module parses and expands such a command line without
touching a file or the GPU: ``sweep_error`` says why a command line cannot run, ``expand`` turns it into per-model split times, band
bounds and parameter vectors, ``structure_error`` is SetModel's check of one model (MigrationInference.py:85-107 and :229-255 of the
reference), under which the reference would have exited in PrintError.

Every model is the cartesian product of the sweeps in the order given, the first outermost (GNU parallel's order).  Band bounds
follow ``misti_eval_batch``: a band end that names the split's own variable is -1, the candidate's split index (a fractional split
ends at its ceiling, as the single run with that end written in does).  A swept rate of a FIXED band (flag 0) takes a parameter slot
of its own behind the optimised ones: the same double lands in the same rate table as the literal value of a single run."""
from __future__ import annotations

import itertools
import re
from math import ceil

import numpy as np

PLACEHOLDER = re.compile(r"^\{([A-Za-z_][A-Za-z0-9_]*)\}$")


def placeholder(field):
    """The variable a command-line field names (``{NAME}``), or None."""
    m = PLACEHOLDER.match(str(field))
    return m.group(1) if m else None


def split_arg(text):
    """argparse type of the positional split time: a number, or a ``{NAME}`` placeholder kept as text."""
    return text if placeholder(text) else float(text)


split_arg.__name__ = "float"           # argparse names the type in its message: a bad number reads as it always has


def _is_int(v):
    try:
        int(v)
        return True
    except ValueError:
        return False


def _is_float(v):
    try:
        float(v)
        return True
    except ValueError:
        return False


def _optimised(flag):
    """A -mi / -pu flag field is optimised exactly when it reads 1 (SetModel's ``migOpt == 1`` / ``puOpt == 1``); anything else
    is a fixed value."""
    return not placeholder(flag) and _is_int(flag) and int(flag) == 1


def _uses(a):
    """Where every placeholder of the command line stands: {name: set of roles} with roles 'split', 'time' (a band start or an
    end that does not follow the split), 'end_split' (a band end following the split), 'rate_opt', 'rate_fixed'; and the
    placeholders found where none may stand, as (option, field) pairs."""
    uses, bad = {}, []
    split_name = placeholder(a.st) if isinstance(a.st, str) else None
    if split_name:
        uses.setdefault(split_name, set()).add("split")
    for el in a.mi:
        for f in (0, 4):
            if placeholder(el[f]):
                bad.append(("-mi", el[f]))
        for f in (1, 2):
            n = placeholder(el[f])
            if n:
                uses.setdefault(n, set()).add("end_split" if f == 2 and n == split_name else "time")
        n = placeholder(el[3])
        if n:
            uses.setdefault(n, set()).add("rate_opt" if _optimised(el[4]) else "rate_fixed")
    for el in a.pu:
        for f in el:
            if placeholder(f):
                bad.append(("-pu", f))
    return uses, bad


def sweep_error(a):
    """Why the sweep on this command line cannot run - one line, checked before any file is read or the GPU is touched - or None
    (also for a command line without placeholders and without --sweep: it runs as it always has)."""
    uses, bad = _uses(a)
    sweeps = a.sweep or []
    if not sweeps and not uses and not bad:
        return None
    for el in a.pu:
        if any(placeholder(f) for f in el):
            return "-pu %s: a pulse takes no placeholder (per-candidate pulse times do not exist in the kernel)" % " ".join(el)
    if bad:
        return "%s ... %s: placeholders stand in the split time and in the start, end and rate fields of -mi only" % bad[0]
    names = []
    for sw in sweeps:
        if not placeholder("{%s}" % sw[0]):
            return "--sweep %s: a sweep variable is a name (letters, digits, _)" % sw[0]
        if len(sw) < 2:
            return "--sweep %s: no values" % sw[0]
        if sw[0] in names:
            return "--sweep %s: the name is declared twice" % sw[0]
        names.append(sw[0])
    for n in uses:
        if n not in names:
            return "{%s} is used but not declared: add --sweep %s V1 V2 ..." % (n, n)
    for n in names:
        if n not in uses:
            return "--sweep %s: the name is declared but {%s} is used nowhere" % (n, n)
    if a.grid_st:
        return "--sweep and --grid-st exclude each other: write the split time as {st} and add --sweep st A A+1 ... B"
    if a.grid_mi:
        return "--sweep and --grid-mi exclude each other: write the rate of that -mi as {NAME} and add --sweep NAME V1 V2 ..."
    if a.gpus > 1 or a.devices:
        return "--sweep runs on one GPU (--device): the sharded gathers of --gpus / --devices take no band bounds"
    values = dict((sw[0], sw[1:]) for sw in sweeps)
    for n, roles in uses.items():
        if roles & {"rate_opt", "rate_fixed"} and roles - {"rate_opt", "rate_fixed"}:
            return "{%s} stands in a rate field and in a time field: a variable is either a time or a rate" % n
        for v in values[n]:
            if "time" in roles and not _is_int(v):
                return "--sweep %s: %s is not an integer, and {%s} is a band start or end (the reference reads them with int())" % (n, v, n)
            if not _is_float(v):
                return "--sweep %s: %s is not a number" % (n, v)
        if a.grid_solve and "rate_fixed" in roles:
            return ("--grid-solve: {%s} is the rate of a fixed band (flag 0); with --grid-solve a rate placeholder stands only in an "
                    "optimised band (flag 1), whose values become the starts" % n)
    optimised = [("-mi", el) for el in a.mi if _optimised(el[4])] + [("-pu", el) for el in a.pu if _optimised(el[3])]
    if a.grid_solve and not optimised:
        return "--grid-solve needs at least one optimised parameter (-mi ... 1 or -pu ... 1)"
    if not a.grid_solve and optimised:
        # an evaluation would print the MiSTI.py:240 line of a model that was never fitted: the reference optimises it
        return ("%s %s is optimised (flag 1): --sweep alone evaluates fixed models; add --grid-solve to fit every model, or fix the "
                "rate (flag 0)" % (optimised[0][0], " ".join(optimised[0][1])))
    return None


class Plan:
    """The expanded sweep.  Per model m (M models, the product of the model variables in --sweep order, first outermost):
    ``assign[m]`` {name: value text}, ``split[m]``, ``bounds[m][n_band][2]`` (int32, end -1 = the model's split index),
    ``params[m][n_param]`` (the optimised parameters first - ``k`` of them, -mi then -pu as the single run orders them - then one
    slot per swept fixed rate), ``mi[m]`` (the -mi options with the values written in: what the result line prints).
    ``starts[Q][k]`` (--grid-solve): the product of the rate variables, the initial values elsewhere.  ``bands`` / ``pulses``: the
    Engine's records (band bounds of model 0; every batch passes its own).  ``values[m][v]``: model m's value of the model
    variable ``model_names[v]``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_model(self):
        return len(self.split)

    def engine_bands(self, m=0):
        """The Engine's band records with model m's bounds (misti_create checks them: any VALID model's will do)."""
        return [(p, int(self.bounds[m, b, 0]), int(self.bounds[m, b, 1]), v, q) for b, (p, _, _, v, q) in enumerate(self.bands)]


def expand(a, solve=None):
    """Expand a command line that passed ``sweep_error``.  ``solve`` (default: ``a.grid_solve``): the rate variables make the
    starts of every model instead of a model axis."""
    solve = a.grid_solve if solve is None else solve
    sweeps = [(sw[0], list(sw[1:])) for sw in (a.sweep or [])]
    uses, _ = _uses(a)
    rate_names = [n for n, _ in sweeps if uses[n] & {"rate_opt", "rate_fixed"}]
    model_names = [n for n, _ in sweeps if not (solve and n in rate_names)]
    vals = dict(sweeps)
    split_name = placeholder(a.st) if isinstance(a.st, str) else None
    # parameter slots: optimised -mi, optimised -pu, then the swept fixed rates
    k = 0
    band_param = []
    for el in a.mi:
        if _optimised(el[4]):
            band_param.append(k)
            k += 1
        else:
            band_param.append(None)
    pulses = []
    for el in a.pu:
        pop, t, val, opt = int(el[0]) - 1, int(el[1]), float(el[2]), _optimised(el[3])
        pulses.append((pop, t, val, k if opt else -1))
        if opt:
            k += 1
    n_param = k
    for b, el in enumerate(a.mi):
        if band_param[b] is None and placeholder(el[3]):
            band_param[b] = n_param
            n_param += 1
    bands = [(int(el[0]) - 1, 0, 0, 0.0 if placeholder(el[3]) else float(el[3]), -1 if band_param[b] is None else band_param[b])
             for b, el in enumerate(a.mi)]

    def value(field, env):
        n = placeholder(field)
        return env[n] if n in env else field          # (--grid-solve: a rate placeholder stays, its values are the starts)

    def param_vector(env):
        p = np.zeros(n_param)
        for b, el in enumerate(a.mi):
            if band_param[b] is not None:
                p[band_param[b]] = float(value(el[3], env))
        for q, el in enumerate(a.pu):
            if _optimised(el[3]):
                p[pulses[q][3]] = float(el[2])
        return p

    assign, split, bounds, params, mi = [], [], [], [], []
    for combo in itertools.product(*[vals[n] for n in model_names]):
        env = dict(zip(model_names, combo))
        assign.append(env)
        split.append(float(value(a.st, env)) if split_name else float(a.st))
        bb = []
        for el in a.mi:
            start = int(value(el[1], env))
            end = -1 if split_name and placeholder(el[2]) == split_name else int(value(el[2], env))
            bb.append((start, end))
        bounds.append(bb)
        params.append(param_vector(env) if not solve else np.zeros(n_param))
        mi.append([[value(f, env) for f in el] for el in a.mi])
    starts = None
    if solve:
        rows = []
        for combo in itertools.product(*[vals[n] for n in rate_names]):
            rows.append(param_vector(dict(zip(rate_names, combo)))[:k])
        starts = np.array(rows, dtype=float).reshape(-1, k)
    M = len(split)
    return Plan(names=[n for n, _ in sweeps], model_names=model_names, rate_names=rate_names, assign=assign,
                split=np.array(split, dtype=float), bounds=np.array(bounds, dtype=np.int32).reshape(M, len(a.mi), 2),
                params=np.array(params, dtype=float).reshape(M, n_param), k=k, n_param=n_param, bands=bands, pulses=pulses, mi=mi,
                starts=starts, values=np.array([[float(env[n]) for n in model_names] for env in assign], dtype=float).reshape(M, len(model_names)))


def structure_error(split, bounds, pops, sample_date, numT):
    """SetModel's verdict on one model (``bounds[n_band][2]``, end -1 = the split index; ``pops`` 0/1 per band), as the reference's
    constructor reaches it (MigrationInference.py:85-107, :229-255) on a grid of ``numT`` intervals: the PrintError text under which
    it would have exited, or None.  A band end beyond the grid is IndexError there."""
    s = int(split)
    frac = split % 1
    if split < sample_date:
        return "cannot initialise class with split time being more recent than sample date."
    if s - 1 > numT - 1:
        return "Invalid value for split time, cannot create Migration class instance."
    if frac != 0.0 and s >= numT - 1:
        return "split time %r cuts no interval of the grid" % split
    n_grid = numT + (1 if frac != 0.0 else 0)
    split_index = int(ceil(split))
    taken = set()
    for (start, end), pop in zip(bounds, pops):
        end = split_index if end == -1 else end
        if start < sample_date:
            return "Migration start (%d) should be larger than or equal to sample date (%d)." % (start, sample_date)
        if end <= start:
            return "Migration start (%d) should be strictly less than migration end (%d)." % (start, end)
        if end > n_grid:
            return "Migration end (%d) is beyond the last time interval (%d)." % (end, n_grid)
        cells = {(pop, t) for t in range(start, end)}
        if cells & taken:
            return "Migration rate intervals should not overlap."
        taken |= cells
    return None
