"""Device assembly of every solver instance group, and the comparison of two trees' dumps: the
check that a change to the launch side (the instance list, the kernels' templates) left the
device code as it was.  No GPU: hipcc cross-compiles.

    python tools/inst_asm.py dump DIR [--root TREE] [--groups N] [--jobs J]
    python tools/inst_asm.py compare DIR_A DIR_B [--out FILE]

dump writes DIR/inst<g>.s for every group g of TREE's mpcg_wide_inst.hip (TREE: this checkout;
N: build.N_INST), with the product's flags (mpc_ros_amd/build.py compile_flags).  compare
prints one line per group and exits 1 if any group differs.  Ignored in the comparison: the
__hip_cuid_ lines (a hash of the source text) and the resume kernels' symbol names (every
mangled name of a k_resume_wide* template reads K_RESUME).
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mpc_ros_amd import build  # noqa: E402


def dump(out, root, groups, jobs):
    os.makedirs(out, exist_ok=True)
    src = os.path.join(root, "mpc_ros_amd", "csrc", "mpcg_wide_inst.hip")
    flags = [f for f in build.compile_flags(root) if not f.startswith("-Rpass")]

    def cc(g):
        cmd = [build.hipcc(), "-S", "--cuda-device-only"] + flags + [f"-DMPCG_INST={g}", src, "-o",
                                                                      os.path.join(out, f"inst{g}.s")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        return g, r

    with ThreadPoolExecutor(jobs) as ex:
        for g, r in ex.map(cc, groups):
            if r.returncode != 0:
                raise SystemExit(f"group {g}: hipcc failed\n{r.stderr}")
            print(f"group {g}: dumped", flush=True)


RESUME_SYM = re.compile(r"_ZN4mpcg\d+k_resume_wide\w*")


def normal(path):
    return [RESUME_SYM.sub("K_RESUME", line) for line in open(path) if "__hip_cuid_" not in line]


def compare(a, b, out):
    names = sorted((f for f in os.listdir(a) if re.fullmatch(r"inst\d+\.s", f)), key=lambda f: int(f[4:-2]))
    report, bad = [], 0
    if names != sorted((f for f in os.listdir(b) if re.fullmatch(r"inst\d+\.s", f)), key=lambda f: int(f[4:-2])):
        raise SystemExit("the two directories hold different groups")
    for f in names:
        la, lb = normal(os.path.join(a, f)), normal(os.path.join(b, f))
        if la == lb:
            report.append(f"group {f[4:-2]}: {len(la)} lines, 0 differing")
            continue
        bad += 1
        d = [x for x in difflib.unified_diff(la, lb, n=0, lineterm="") if x[:1] in "+-" and x[:3] not in ("+++", "---")]
        report.append(f"group {f[4:-2]}: {len(la)} / {len(lb)} lines, {len(d)} DIFFERING")
        report += ["    " + x.rstrip() for x in d[:20]]
    report.append(f"{len(names)} groups, {bad} differing")
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("dir")
    d.add_argument("--root", default=build.ROOT)
    d.add_argument("--groups", type=int, default=build.N_INST)
    d.add_argument("--only", help="comma-separated groups (default: all)")
    d.add_argument("--jobs", type=int, default=max(1, min(os.cpu_count() or 1, 16)))
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    c.add_argument("--out")
    args = ap.parse_args()
    if args.cmd == "dump":
        only = [int(g) for g in args.only.split(",")] if args.only else range(args.groups)
        dump(args.dir, os.path.abspath(args.root), only, args.jobs)
    else:
        sys.exit(compare(args.a, args.b, args.out))
