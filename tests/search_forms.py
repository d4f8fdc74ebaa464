"""What tests/test_search_cpu.py and tests/test_gpu_search.py share: one set of search fields (numpy arrays and numbers, named as
misti_search_t / misti_hops_t name them) turned into a descriptor for misti_search, or into the argument list of one of the ten older
entry points - the order of THAT list read from the symbol's prototype in include/misti_hip.h, so nothing here restates it."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

LEGACY = ("misti_nm_solve", "misti_nm_solve_rows", "misti_nm_solve_bounds", "misti_nm_solve_pulses", "misti_nm_solve_split",
          "misti_nm_solve_box", "misti_basinhopping", "misti_basinhopping_rows", "misti_basinhopping_split", "misti_basinhopping_box")
# prototype names that are a descriptor field under another name
RENAMED = {"jsfs_row": "jsfs", "nm_maxiter": "maxiter"}
HOP_OUTPUTS = ("nfev", "failures", "accepted")


def header():
    return open(os.path.join(ROOT, "include", "misti_hip.h")).read()


def prototype_names(symbol):
    """The argument names of ``symbol``'s prototype behind ``ctx``, in order."""
    m = re.search(r"^int %s\s*\(([^;]*)\);" % symbol, header(), re.M)
    assert m, "no prototype of " + symbol
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names[0] == "ctx"
    return names[1:]


def struct_fields(name):
    """The field names the header declares for ``name`` (misti_search_t / misti_hops_t), in order."""
    hdr = header()
    m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr) or re.search(r"^struct %s \{([^}]*)\};" % name, hdr, re.M)
    assert m, "no definition of " + name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()]


def _addr(v):
    return v.ctypes.data if isinstance(v, np.ndarray) else v


def descriptor(f):
    """``f`` as a ``_lib.Search`` (with its ``_lib.Hops`` where ``f["hops"]`` is a dict).  The arrays stay the caller's."""
    from misti_amd import _lib
    q = _lib.Search(size=C.sizeof(_lib.Search))
    for k, v in f.items():
        if k != "hops":
            setattr(q, k, _addr(v))
    if f.get("hops") is not None:
        h = _lib.Hops(**{k: _addr(v) for k, v in f["hops"].items()})
        q._hops = h                                        # keeps the record alive with its descriptor
        q.hops = C.pointer(h)
    return q


def is_hop_form(symbol):
    return "basinhopping" in symbol


def form_of(symbol, full):
    """The fields of ``full`` that ``symbol`` takes - the descriptor that symbol is: every field its prototype does not name is
    absent (NULL / 0), the split mode follows from which split argument it has and whether that is given."""
    from misti_amd import _lib
    names = [RENAMED.get(n, n) for n in prototype_names(symbol)]
    hop = is_hop_form(symbol)
    f = {k: v for k, v in full.items() if k in names and k != "hops" and not (hop and k in ("nit", "nfev", "status"))}
    if "split_time" in names:
        f["split"], f["n_rep"] = _lib.SPLIT_ONE, 1
    else:
        f["split"] = _lib.SPLIT_PER_START if f.get("split_times") is not None else _lib.SPLIT_FITTED
    if hop:
        f["hops"] = dict(full["hops"])
    return f


def legacy_args(symbol, f):
    """The argument list of ``symbol`` behind ``ctx`` for the fields ``f`` (as ``form_of`` made them)."""
    hop = is_hop_form(symbol)
    args = []
    for n in prototype_names(symbol):
        n = RENAMED.get(n, n)
        src = f["hops"] if hop and (n in f["hops"] or n in HOP_OUTPUTS) else f
        args.append(_addr(src.get(n)))
    return args
