#!/usr/bin/env python3
"""Instruction census of the active-set sweeps (pmpc_amd/csrc/kernels_as.hip), from the compiler's gfx950 assembly.  No GPU needed.

    python tools/isa_census.py                      # the four sweeps of the flagship shape, every inner loop
    python tools/isa_census.py --resources-all      # + registers / scratch of every kernel of the (12, 4) build
    python tools/isa_census.py --asm FILE.s         # census of an assembly file made earlier (no compile)
    python tools/isa_census.py > profiles/rNN_census_branch.txt

Compiles kernels_as.hip with the Makefile's flags plus -DPMPC_DIAG_DIMS_12_4 --cuda-device-only -S (about a minute) and, for
each innermost loop (a backward branch with no backward branch inside) of the kernels named in KERNELS, counts the instructions
by class.  Classes are told apart by mnemonic PREFIX and operand-size suffix alone; the tool knows no instruction by name.
A loop of a sweep is one stage per trip (MODE 2 / PF2: three stages per trip — the tool prints the MFMA count, which says how
many: the factor stage has 7, the forward stage 4, +1 each with SENS or CONE terms)."""
import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pmpc_amd" / "csrc"

# (title, fragment of the mangled name)
KERNELS = [
    ("full factor sweep            k_bwd_as<12,4,1,false,true,0,double>", "k_bwd_asILi12ELi4ELi1ELb0ELb1ELi0EdE"),
    ("restarted factor sweep       k_bwd_as<12,4,2,true,false,0,double>", "k_bwd_asILi12ELi4ELi2ELb1ELb0ELi0EdE"),
    ("first-round forward sweep    k_fwd_as<12,4,true,true,false,double,true>", "k_fwd_asILi12ELi4ELb1ELb1ELb0EdLb1EE"),
    ("later-round forward sweep    k_fwd_as<12,4,false,true,false,double,true>", "k_fwd_asILi12ELi4ELb0ELb1ELb0EdLb1EE"),
]

CLASSES = ["vector", "mfma", "scalar", "lds", "global"]
SUB = ["select", "mov32", "mov64", "dpp_mov", "readlane", "permlane", "addr64_add", "fp64_arith", "other"]


def makefile_flags():
    """CXXFLAGS of pmpc_amd/csrc/Makefile (ARCH and EXTRA expanded to their defaults)."""
    text = (CSRC / "Makefile").read_text()
    m = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = m.group(1).replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    return hipcc, flags


def compile_asm(out, extra):
    hipcc, flags = makefile_flags()
    cmd = [hipcc, *flags, "-DPMPC_DIAG_DIMS_12_4", *extra, "--cuda-device-only", "-S", "kernels_as.hip", "-o", str(out)]
    subprocess.check_call(cmd, cwd=CSRC)


def classify(mn, ops):
    """-> (class, vector sub-class or None), by prefix / suffix of the mnemonic only."""
    if mn.startswith("v_mfma") or mn.startswith("v_smfma"):
        return "mfma", None
    if mn.startswith("v_"):
        if mn.startswith("v_cndmask"):
            sub = "select"
        elif mn.startswith("v_readlane") or mn.startswith("v_readfirstlane"):
            sub = "readlane"
        elif mn.startswith("v_permlane"):
            sub = "permlane"
        elif mn.startswith("v_mov") and ("dpp" in mn or re.search(r"\b(quad_perm|row_\w+|wave_\w+):?", ops)):
            sub = "dpp_mov"
        elif mn.startswith("v_mov_b64"):
            sub = "mov64"
        elif mn.startswith("v_mov_b32") or mn.startswith("v_accvgpr"):
            sub = "mov32"
        elif mn.startswith("v_lshl_add_u64") or mn.startswith("v_add_co") or mn.startswith("v_addc_co"):
            sub = "addr64_add"
        elif re.search(r"_f64(_e32|_e64)?$", mn) and not mn.startswith("v_cmp"):
            sub = "fp64_arith"
        else:
            sub = "other"
        return "vector", sub
    if mn.startswith("s_"):
        return "scalar", None
    if mn.startswith("ds_"):
        return "lds", None
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global", None
    return None, None


INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\s*(.*?)\s*(?://.*|;.*)?$")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^s_c?branch\w*$")


def kernels_of(lines):
    """name -> (first line, last line) of the function body, and name -> resources from its .amdhsa_kernel block."""
    bodies, res, cur, start = {}, {}, None, 0
    for n, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur, start = m.group(1), n
        elif ln.startswith(".Lfunc_end") and cur:
            bodies[cur] = (start, n)
            cur = None
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kn = m.group(1)
            res[kn] = {}
        m = re.match(r"^\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size|accum_offset)\s+(\d+)", ln)
        if m and res:
            res[kn][m.group(1)] = int(m.group(2))
    return bodies, res


def inner_loops(lines, lo, hi):
    labels = {}
    for n in range(lo, hi):
        m = LABEL.match(lines[n])
        if m:
            labels[m.group(1)] = n
    back = []
    for n in range(lo, hi):
        m = INSN.match(lines[n])
        if m and BRANCH.match(m.group(1)):
            tgt = m.group(2).split()[0] if m.group(2) else ""
            if tgt in labels and labels[tgt] <= n:
                back.append((labels[tgt], n, tgt))
    return [b for b in back if not any(o is not b and b[0] <= o[0] and o[1] <= b[1] for o in back)]


def census(lines, lo, hi):
    cls = dict.fromkeys(CLASSES, 0)
    sub = dict.fromkeys(SUB, 0)
    for n in range(lo, hi + 1):
        m = INSN.match(lines[n])
        if not m or m.group(1).startswith("."):
            continue
        c, s = classify(m.group(1), m.group(2))
        if c:
            cls[c] += 1
        if s:
            sub[s] += 1
    return cls, sub


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="assembly file to read instead of compiling")
    ap.add_argument("--keep", help="write the assembly here")
    ap.add_argument("--resources-all", action="store_true", help="registers and scratch of every kernel in the file")
    ap.add_argument("-D", dest="defs", action="append", default=[], help="extra -D for the compile (A/B builds)")
    args = ap.parse_args()
    if args.asm:
        path = Path(args.asm)
    else:
        path = Path(args.keep) if args.keep else Path(tempfile.mkdtemp()) / "kernels_as.s"
        compile_asm(path, ["-D" + d for d in args.defs])
    lines = path.read_text().splitlines()
    bodies, res = kernels_of(lines)
    print("# instruction census of the active-set sweeps, (xdim, udim) = (12, 4), gfx950; counts per loop TRIP")
    for title, frag in KERNELS:
        names = [k for k in bodies if frag in k]
        if len(names) != 1:
            print(f"{title}: {len(names)} kernels match {frag}", file=sys.stderr)
            return 1
        k = names[0]
        r = res.get(k, {})
        print(f"\n{title}")
        print(f"  next_free_vgpr {r.get('next_free_vgpr')}  next_free_sgpr {r.get('next_free_sgpr')}  scratch bytes {r.get('private_segment_fixed_size')}")
        lo, hi = bodies[k]
        for (a, b, tgt) in inner_loops(lines, lo, hi):
            cls, sub = census(lines, a, b)
            print(f"  loop {tgt}: " + "  ".join(f"{c} {cls[c]}" for c in CLASSES))
            print("    vector: " + "  ".join(f"{s} {sub[s]}" for s in SUB))
    if args.resources_all:
        print("\n# every kernel: next_free_vgpr next_free_sgpr scratch_bytes name")
        for k in sorted(res):
            r = res[k]
            print(f"{r.get('next_free_vgpr'):4d} {r.get('next_free_sgpr'):4d} {r.get('private_segment_fixed_size'):5d}  {k}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
