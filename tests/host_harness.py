"""The native check programs of tests/native/ for the test modules: the one compile line, and the
stdin of the wide_*_check programs (tests/native/host_wave.h describes the format).

A plain module: the test modules import it; it is no conftest and holds no fixture.
"""
from __future__ import annotations

import atexit
import itertools
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
_dir = tempfile.mkdtemp(prefix="mpcg_native_")  # the session's executables
atexit.register(shutil.rmtree, _dir, ignore_errors=True)
_built = {}  # (program, flags) -> executable
_serial = itertools.count()


def build(program, *flags) -> str:
    """tests/native/<program>.cpp compiled with the flags, once per (program, flags) and session,
    into a temporary directory; the executable's path.  The flags follow -O2, so an -O level
    among them (the sanitizer build's) replaces it."""
    key = (program, flags)
    if key not in _built:
        exe = os.path.join(_dir, f"{program}_{next(_serial)}")
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-w", "-pthread", *flags, "-o", exe,
                               os.path.join(NATIVE, program + ".cpp")])
        _built[key] = exe
    return _built[key]


def build_all(program, flag_sets) -> list:
    """build(program, *flags) of every flags in flag_sets, the compilers running side by side."""
    with ThreadPoolExecutor(len(flag_sets)) as pool:
        return list(pool.map(lambda flags: build(program, *flags), flag_sets))


# fields of the oracle's IpmOpts that are no option of the device core
ORACLE_ONLY = ("honor_original_bounds", "print_level", "kkt_structured", "refine_steps")


def opts_line(o, filter_cap=64) -> str:
    """The harness's Ipopt-option lines from an oracle IpmOpts: every field under its own name
    (same values both sides; restoration = 0 is the core's no_restoration = 1), closed by "end".
    The harness refuses a name the core does not have."""
    lines = [f"filter_cap {int(filter_cap)}"]
    for name, _ in o._fields_:
        if name in ORACLE_ONLY:
            continue
        if name == "restoration":
            lines.append(f"no_restoration {0 if o.restoration else 1}")
        else:
            lines.append(f"{name} {getattr(o, name)!r}")
    return "\n".join(lines + ["end"])


def harness_stdin(P, state, coeffs, o, options) -> str:
    """The harness's input: the two problem lines, the option lines, the problems."""
    hdr = (f"{int(P['STEPS'])} {P['DT']!r} {P['REF_CTE']!r} {P['REF_ETHETA']!r} {P['REF_V']!r} {P['W_CTE']!r} "
           f"{P['W_EPSI']!r} {P['W_V']!r} {P['W_ANGVEL']!r} {P['W_A']!r} {P['W_DANGVEL']!r} {P['W_DA']!r} "
           f"{P['ANGVEL']!r} {P['MAXTHR']!r} {P['BOUND']!r} {o.tol!r} {o.max_iter}\n"
           f"{int(P.get('MODEL', 0))} {float(P.get('LF', 0.5))!r}\n{options}\n{len(state)}\n")
    body = "\n".join(" ".join(repr(float(v)) for v in np.concatenate([state[b], coeffs[b]]))
                     for b in range(len(state)))
    return hdr + body + "\n"
