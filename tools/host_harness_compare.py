#!/usr/bin/env python3
"""The five wide_*_check programs of tests/native/ at a parent commit against the working tree:
the same bytes on stdout (and, for the refusals, the same stderr and exit status) for a fixed set
of inputs that takes every path through the shared part (tests/native/host_wave.h).

    python tools/host_harness_compare.py [--parent REV] [--out profiles/host/harness_compare.txt]

Both trees' programs are built into a temporary directory (the parent's sources by git archive),
every input is run with MPCG_HOST_THREADS=1 and with the default, and one line per program, flags
and input goes to the output: the sha256 of the parent's and of the tree's stdout.  Exit status 1
if any pair differs.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from host_harness import harness_stdin, opts_line  # noqa: E402
from oracle import pyoracle as O  # noqa: E402
from test_core_host import fp32_opts  # noqa: E402
from test_solution_host import fixture_set  # noqa: E402

F32, F0, F3 = ("-DHOST_T=float",), ("-DMPCG_FUSE=0",), ("-DMPCG_FUSE=3",)
BUILDS = [("wide_host_check", ()), ("wide_host_check", F32), ("wide_sol_check", ()), ("wide_start_check", ())]
BUILDS += [(p, ty + f) for p, alt in (("wide_fused_check", F0), ("wide_slack_check", F3))
           for ty in ((), F32) for f in ((), alt)]
TWO = {"MPCG_HOST_TWO_PHASE": "1"}


def compile_tree(tree, out):
    """{(program, flags): executable} of the tree's programs."""
    def one(build):
        prog, flags = build
        exe = os.path.join(out, prog + "".join(flags).replace("-D", "_").replace("=", ""))
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-w", "-pthread", *flags, "-o", exe,
                               os.path.join(tree, "tests", "native", prog + ".cpp")])
        return exe
    with ThreadPoolExecutor(os.cpu_count() or 4) as pool:
        return dict(zip(BUILDS, pool.map(one, BUILDS)))


def rows(name, sel, model=None):
    P, g = fixture_set(name)
    if model is not None:
        P = dict(P, MODEL=model, LF=0.5)
    return P, np.ascontiguousarray(g["state"][sel]), np.ascontiguousarray(g["coeffs"][sel])


def text(P, st, cf, o=None, options=None):
    o = o if o is not None else O.ref_opts(int(P["STEPS"]))
    return harness_stdin(P, st, cf, o, options if options is not None else opts_line(o))


def start_tail(N, modes, starts, mu0=1e-4, cold_scaling=0):
    tail = [str(cold_scaling)]
    for m, s in zip(modes, starts):
        tail += [f"{m} {mu0!r}", " ".join(repr(float(v)) for v in s)]
    return "\n".join(tail) + "\n"


def cases(parent):
    """(program, flags, input name, stdin, environment): the issue's table, then the refusals."""
    inf = rows("infinity", np.r_[0:8, 256:260])
    inf4 = rows("infinity", slice(0, 4))
    n40 = rows("variants_N40", slice(0, 4))
    N = int(inf4[0]["STEPS"])
    out = [("wide_host_check", (), "infinity_N20[0:8,256:260]", text(*inf), {}),
           ("wide_host_check", (), "variants_N40[0:3]", text(*rows("variants_N40", slice(0, 3))), {}),
           ("wide_host_check", (), "resto_N65[0]", text(*rows("resto_N65", [0])), {}),
           ("wide_host_check", (), "features_bicycle[4,5]", text(*rows("bicycle", [4, 5], model=1)), {}),
           ("wide_host_check", (), "variants_small_bound[0:2]", text(*rows("variants_small_bound", slice(0, 2))), {}),
           ("wide_host_check", F32, "infinity_N20[0:4],FP32_OPTIONS", text(*inf4, fp32_opts(O, N)), {}),
           ("wide_host_check", (), "two-phase,infinity_N20[0:4]", text(*inf4, fp32_opts(O, N)), TWO),
           ("wide_host_check", (), "two-phase,variants_N40[0:4]", text(*n40, fp32_opts(O, 40)), TWO),
           ("wide_sol_check", (), "infinity_N20[0:4]", text(*inf4), {})]
    # the start records: the parent's cold solutions of the four rows
    ne = 3 * (8 * N - 2) + 6 * N
    zero = np.zeros((4, ne))
    cold = text(*inf4) + start_tail(N, [0] * 4, zero)
    sol = np.array([r.split() for r in run(parent["wide_start_check", ()], cold, {})[0].decode().splitlines()],
                   dtype=np.float64)[:, 10 + 3 * N:]
    bad = sol.copy()
    bad[1, 3 * N + 2] = np.nan
    out += [("wide_start_check", (), "infinity_N20[0:4],COLD", cold, {}),
            ("wide_start_check", (), "infinity_N20[0:4],PRIMAL", text(*inf4) + start_tail(N, [1] * 4, sol), {}),
            ("wide_start_check", (), "infinity_N20[0:4],FULL", text(*inf4) + start_tail(N, [2] * 4, sol), {}),
            ("wide_start_check", (), "infinity_N20[0:4],mixed,NaN-record", text(*inf4) + start_tail(N, [1, 1, 2, 0], bad), {}),
            ("wide_start_check", (), "infinity_N20[0:4],PRIMAL,cold-scaling", text(*inf4) + start_tail(N, [1] * 4, sol, cold_scaling=1), {})]
    for prog, alt in (("wide_fused_check", F0), ("wide_slack_check", F3)):
        for ty in ((), F32):
            o = fp32_opts(O, N) if ty else None
            out += [(prog, ty + f, "infinity_N20[0:4]", text(*inf4, o), {}) for f in ((), alt)]
    # the refusals (stdout, stderr and the exit status are compared)
    o = O.ref_opts(N)
    unknown = text(*inf4, o, "no_such_option 1\n" + opts_line(o))
    full = text(*inf4)
    in_options = "\n".join(full.split("\n")[:5]) + "\n"  # (the two parameter lines, three options, no "end")
    in_rows = full[:full.rindex(" ")] + "\n"             # (the last problem's last value is missing)
    for prog in ("wide_host_check", "wide_sol_check", "wide_start_check", "wide_fused_check", "wide_slack_check"):
        out += [(prog, (), "refusal:unknown-option", unknown, {}), (prog, (), "refusal:truncated-options", in_options, {})]
        if prog != "wide_host_check":  # (the parent's did not check its problem rows; the tree's refuses like the others)
            out.append((prog, (), "refusal:truncated-rows", in_rows, {}))
    out += [(prog, (), "refusal:N40", text(*n40), {}) for prog in ("wide_fused_check", "wide_slack_check")]
    return out


def run(exe, stdin, env):
    r = subprocess.run([exe], input=stdin.encode(), capture_output=True, env=dict(os.environ, **env))
    return r.stdout, r.stderr, r.returncode


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host", "harness_compare.txt"))
    a = ap.parse_args()
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", a.parent], text=True).strip()
    with tempfile.TemporaryDirectory() as tmp:
        ptree = os.path.join(tmp, "parent")
        os.makedirs(ptree)
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", a.parent, "tests/native", "mpc_ros_amd/csrc"],
                              stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", ptree], stdin=ar.stdout)
        assert ar.wait() == 0
        for d in ("pb", "tb"):
            os.makedirs(os.path.join(tmp, d))
        parent, tree = compile_tree(ptree, os.path.join(tmp, "pb")), compile_tree(ROOT, os.path.join(tmp, "tb"))
        lines = [f"# tests/native wide_*_check programs: parent {rev} against the tree, by tools/host_harness_compare.py",
                 "# program [flags] | input | sha256 of the parent's stdout | of the tree's | verdict",
                 "# (every input run with MPCG_HOST_THREADS=1 and with the default: the verdict covers both;",
                 "#  a refusal's verdict covers stderr and the exit status too)"]
        n_bad = 0
        for prog, flags, name, stdin, env in cases(parent):
            got = [run(exes[prog, flags], stdin, dict(env, **th))
                   for exes in (parent, tree) for th in ({"MPCG_HOST_THREADS": "1"}, {})]
            refusal = name.startswith("refusal:")
            same = all(g == got[0] for g in got[1:])
            ok = same and (got[0][2] != 0 if refusal else got[0][2] == 0 and len(got[0][0]) > 0)
            n_bad += not ok
            sha = [hashlib.sha256(g[0]).hexdigest()[:16] for g in (got[0], got[2])]
            note = f" exit {got[0][2]} stderr {got[0][1].decode().strip()!r}" if refusal else f" {len(got[0][0])} bytes"
            lines.append(f"{prog}{' ' + ' '.join(flags) if flags else ''} | {name}{' ' + ' '.join(f'{k}={v}' for k, v in env.items()) if env else ''}"
                         f" | {sha[0]} | {sha[1]} | {'same' if ok else 'DIFFERENT'}{note}")
            print(lines[-1], flush=True)
        lines.append(f"# {len(lines) - 4} inputs, {n_bad} differing")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main())
