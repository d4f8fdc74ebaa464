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
of its own behind the optimised ones: the same double lands in the same rate table as the literal value of a single run.

``--sweep-pu NAME V1 V2 ...`` declares a variable of the pulses: ``{NAME}`` stands in the time field or in the fraction field of
``-pu`` (never both, and nowhere else) - the same recipe with ``-pu 2 {t} {f} 0`` in the place of a band, "when did the admixture
pulse happen".  The models are the product of the --sweep variables in their order, then the --sweep-pu variables in theirs, the
last innermost; a pulse time is a per-candidate time of ``misti_eval_batch_pulses``, a swept fixed fraction a parameter slot behind
those of the swept fixed rates."""
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
    'pu_time', 'pu_frac_opt', 'pu_frac_fixed' (the time and the fraction field of a -pu); and the placeholders found where none may
    stand, as (option, field) pairs."""
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
        for f in (0, 3):
            if placeholder(el[f]):
                bad.append(("-pu", el[f]))
        n = placeholder(el[1])
        if n:
            uses.setdefault(n, set()).add("pu_time")
        n = placeholder(el[2])
        if n:
            uses.setdefault(n, set()).add("pu_frac_opt" if _optimised(el[3]) else "pu_frac_fixed")
    return uses, bad


MI_ROLES = {"split", "time", "end_split", "rate_opt", "rate_fixed"}
PU_ROLES = {"pu_time", "pu_frac_opt", "pu_frac_fixed"}
RATE_ROLES = {"rate_opt", "rate_fixed", "pu_frac_opt", "pu_frac_fixed"}


def _pu_sweeps(a):
    return getattr(a, "sweep_pu", None) or []


def sweep_error(a):
    """Why the sweep on this command line cannot run - one line, checked before any file is read or the GPU is touched - or None
    (also for a command line without placeholders and without --sweep: it runs as it always has)."""
    uses, bad = _uses(a)
    sweeps = a.sweep or []
    pu_sweeps = _pu_sweeps(a)
    if not sweeps and not pu_sweeps and not uses and not bad:
        return None
    plain = [sw[0] for sw in sweeps]
    for el in a.pu:
        if any(placeholder(f) in plain for f in el):
            return ("-pu %s: a pulse takes no placeholder (per-candidate pulse times and fractions are swept with their own option: "
                    "declare the variable with --sweep-pu NAME V1 V2 ..., not with --sweep)" % " ".join(el))
    for opt, f in bad:
        if opt == "-pu":
            return "-pu ... %s: placeholders stand in the time and fraction fields of -pu only" % f
    if bad:
        return "%s ... %s: placeholders stand in the split time and in the start, end and rate fields of -mi only" % bad[0]
    names, pu_names = [], []
    for option, group in (("--sweep", sweeps), ("--sweep-pu", pu_sweeps)):
        for sw in group:
            if not placeholder("{%s}" % sw[0]):
                return "%s %s: a sweep variable is a name (letters, digits, _)" % (option, sw[0])
            if len(sw) < 2:
                return "%s %s: no values" % (option, sw[0])
            if sw[0] in names:
                return "%s %s: the name is declared twice" % (option, sw[0])
            names.append(sw[0])
            if option == "--sweep-pu":
                pu_names.append(sw[0])
    for n, roles in uses.items():
        if n not in names:
            option = "--sweep-pu" if roles & PU_ROLES else "--sweep"
            return "{%s} is used but not declared: add %s %s V1 V2 ..." % (n, option, n)
    for n in names:
        if n not in uses:
            return "%s %s: the name is declared but {%s} is used nowhere" % ("--sweep-pu" if n in pu_names else "--sweep", n, n)
    for n in pu_names:
        if uses[n] & MI_ROLES:
            return "--sweep-pu %s: {%s} stands in the time and fraction fields of -pu only (the split time and -mi take --sweep variables)" % (n, n)
        if "pu_time" in uses[n] and uses[n] - {"pu_time"}:
            return "--sweep-pu %s: {%s} stands in a time field and in a fraction field: a variable is either a pulse time or a pulse fraction" % (n, n)
    if a.grid_st:
        return "--sweep and --grid-st exclude each other: write the split time as {st} and add --sweep st A A+1 ... B"
    if a.grid_mi:
        return "--sweep and --grid-mi exclude each other: write the rate of that -mi as {NAME} and add --sweep NAME V1 V2 ..."
    if a.gpus > 1 or a.devices:
        return "--sweep runs on one GPU (--device): the sharded gathers of --gpus / --devices take no band bounds and no pulse times"
    values = dict((sw[0], sw[1:]) for sw in list(sweeps) + list(pu_sweeps))
    for n, roles in uses.items():
        if roles & {"rate_opt", "rate_fixed"} and roles - {"rate_opt", "rate_fixed"}:
            return "{%s} stands in a rate field and in a time field: a variable is either a time or a rate" % n
        for v in values[n]:
            if "time" in roles and not _is_int(v):
                return "--sweep %s: %s is not an integer, and {%s} is a band start or end (the reference reads them with int())" % (n, v, n)
            if "pu_time" in roles and not _is_int(v):
                return "--sweep-pu %s: %s is not an integer, and {%s} is a pulse time (the reference reads it with int())" % (n, v, n)
            if not _is_float(v):
                return "%s %s: %s is not a number" % ("--sweep-pu" if n in pu_names else "--sweep", n, v)
        if a.grid_solve and "pu_frac_fixed" in roles:
            return ("--grid-solve: {%s} is the fraction of a fixed pulse (flag 0); with --grid-solve a fraction placeholder stands only in "
                    "an optimised pulse (flag 1), whose values become the starts" % n)
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
    ``pulse_times[m][n_pulse]`` (int32: the time of every -pu of model m), ``pulse_values[m][n_pulse]`` (its fraction as written or
    swept; nan where --grid-solve makes starts of it), ``pu[m]`` (the -pu options with the values written in), ``pulse_swept``
    (a --sweep-pu variable stands in a time field: batches pass ``pulse_times``).
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

    def engine_pulses(self, m=0):
        """The Engine's pulse records with model m's times (misti_create checks them: any VALID model's will do)."""
        return [(p, int(self.pulse_times[m, q]), v, k) for q, (p, _, v, k) in enumerate(self.pulses)]


def expand(a, solve=None):
    """Expand a command line that passed ``sweep_error``.  ``solve`` (default: ``a.grid_solve``): the rate variables make the
    starts of every model instead of a model axis."""
    solve = a.grid_solve if solve is None else solve
    sweeps = [(sw[0], list(sw[1:])) for sw in list(a.sweep or []) + list(_pu_sweeps(a))]
    uses, _ = _uses(a)
    rate_names = [n for n, _ in sweeps if uses[n] & RATE_ROLES]
    model_names = [n for n, _ in sweeps if not (solve and n in rate_names)]
    vals = dict(sweeps)
    split_name = placeholder(a.st) if isinstance(a.st, str) else None
    # parameter slots: optimised -mi, optimised -pu, then the swept fixed rates, then the swept fixed pulse fractions
    k = 0
    band_param = []
    for el in a.mi:
        if _optimised(el[4]):
            band_param.append(k)
            k += 1
        else:
            band_param.append(None)
    pulse_param = []
    for el in a.pu:
        if _optimised(el[3]):
            pulse_param.append(k)
            k += 1
        else:
            pulse_param.append(None)
    n_param = k
    for b, el in enumerate(a.mi):
        if band_param[b] is None and placeholder(el[3]):
            band_param[b] = n_param
            n_param += 1
    for q, el in enumerate(a.pu):
        if pulse_param[q] is None and placeholder(el[2]):
            pulse_param[q] = n_param
            n_param += 1
    pulses = [(int(el[0]) - 1, 0 if placeholder(el[1]) else int(el[1]), 0.0 if placeholder(el[2]) else float(el[2]),
               -1 if pulse_param[q] is None else pulse_param[q]) for q, el in enumerate(a.pu)]
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
            if pulse_param[q] is not None:
                p[pulse_param[q]] = float(value(el[2], env))
        return p

    assign, split, bounds, params, mi, pu, pulse_times, pulse_values = [], [], [], [], [], [], [], []
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
        pu.append([[value(f, env) for f in el] for el in a.pu])
        pulse_times.append([int(value(el[1], env)) for el in a.pu])
        pulse_values.append([float("nan") if placeholder(value(el[2], env)) else float(value(el[2], env)) for el in a.pu])
    starts = None
    if solve:
        rows = []
        for combo in itertools.product(*[vals[n] for n in rate_names]):
            rows.append(param_vector(dict(zip(rate_names, combo)))[:k])
        starts = np.array(rows, dtype=float).reshape(-1, k)
    M = len(split)
    return Plan(names=[n for n, _ in sweeps], model_names=model_names, rate_names=rate_names, assign=assign,
                split=np.array(split, dtype=float), bounds=np.array(bounds, dtype=np.int32).reshape(M, len(a.mi), 2),
                params=np.array(params, dtype=float).reshape(M, n_param), k=k, n_param=n_param, bands=bands, pulses=pulses, mi=mi, pu=pu,
                pulse_times=np.array(pulse_times, dtype=np.int32).reshape(M, len(a.pu)),
                pulse_values=np.array(pulse_values, dtype=float).reshape(M, len(a.pu)),
                pulse_swept=any("pu_time" in uses[n] for n, _ in sweeps),
                starts=starts, values=np.array([[float(env[n]) for n in model_names] for env in assign], dtype=float).reshape(M, len(model_names)))


def structure_error(split, bounds, pops, sample_date, numT, pulse_times=None, pulse_values=None):
    """SetModel's verdict on one model (``bounds[n_band][2]``, end -1 = the split index; ``pops`` 0/1 per band; ``pulse_times`` and
    ``pulse_values`` per -pu, nan = a value SetModel never sees), as the reference's constructor reaches it
    (MigrationInference.py:85-107, :229-279) on a grid of ``numT`` intervals: the PrintError text under which it would have exited,
    or None.  A band end or a pulse time beyond the grid is IndexError there."""
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
    seen = set()
    for q, t in enumerate(() if pulse_times is None else pulse_times):
        t = int(t)
        if t < sample_date:
            return "Pulse migration time (%d) should be larger than or equal to sample date (%d)." % (t, sample_date)
        if pulse_values is not None and (pulse_values[q] < 0 or pulse_values[q] > 1):
            return "Pulse migration rate should be between 0 and 1."
        if t >= n_grid:
            return "Pulse migration time (%d) is beyond the last time interval (%d)." % (t, n_grid)
        if t in seen:
            return "Current version allows only single-direction pulse migration at a time."
        seen.add(t)
    return None
