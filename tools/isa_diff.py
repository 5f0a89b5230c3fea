#!/usr/bin/env python3
"""Compare two `make asm` trees (build/asm of two checkouts) per kernel symbol.

    tools/isa_diff.py OLD/build/asm NEW/build/asm [--list]

For every NAME.s: each function symbol's instruction stream and its
.amdhsa_* block, with comments dropped and the compiler's local labels
(.LBB<f>_<n>, .Lfunc_*, .LJTI*, .Ltmp*) renumbered in order of appearance, so a
function that only moved inside its file compares equal.  For every NAME.usage:
the resource remarks per function (registers, scratch, LDS, occupancy) without
their source positions.  Prints one line per file with the counts of symbols
identical, differing, added and removed, then each differing symbol with its
instruction counts before and after and whether its .usage entry changed;
--list also names the identical ones.  It only diffs: it knows nothing about
particular instructions.  Exit status 1 when anything differs."""
import argparse
import os
import re
import subprocess
import sys

LOCAL = re.compile(r"\.L(?:BB\d+_\d+|func_(?:begin|end)\d+|JTI\d+_\d+|tmp\d+|__unnamed_\d+)")
FUNC_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
USAGE = re.compile(r"^\S+:\d+:\d+: remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]$")


def _clean(line):
    """An assembly line without its comment and surrounding blanks."""
    return line.split(";", 1)[0].strip()


def _renumber(lines):
    names = {}

    def repl(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))
    return [LOCAL.sub(repl, l) for l in lines]


def symbols(path):
    """{symbol: (stream lines, amdhsa lines)} of one .s file."""
    out = {}
    name, body, hsa, in_body, in_hsa = None, [], [], False, False
    with open(path) as f:
        for raw in f:
            m = FUNC_TYPE.match(raw)
            if m:
                name, body, hsa, in_body = m.group(1), [], [], False
                continue
            line = _clean(raw)
            if not line or name is None:
                continue
            if line == name + ":":
                in_body = True
            elif line.startswith(".amdhsa_kernel"):
                in_body, in_hsa = False, True
            elif line.startswith(".end_amdhsa_kernel"):
                in_hsa = False
            elif line.startswith(".size") and name in line:
                out[name] = (_renumber(body), hsa)
                name = None
            elif in_hsa:
                hsa.append(line)
            elif in_body and not line.startswith((".section", ".p2align")):
                body.append(line)
    return out


def usage(path):
    """{symbol: [resource remark, ...]} of one .usage file."""
    out, cur = {}, None
    if not os.path.exists(path):
        return out
    with open(path) as f:
        for raw in f:
            m = USAGE.match(raw.rstrip("\n"))
            if not m:
                continue
            text = m.group(1)
            if text.startswith("Function Name:"):
                cur = out.setdefault(text.split(":", 1)[1].strip(), [])
            elif cur is not None:
                cur.append(text)
    return out


def _ninstr(stream):
    return sum(1 for l in stream if not l.endswith(":") and not l.startswith("."))


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                           check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--list", action="store_true", help="name the identical symbols too")
    a = ap.parse_args()
    files = sorted({f for d in (a.old, a.new) for f in os.listdir(d) if f.endswith(".s")})
    differs = False
    details = []
    for f in files:
        po, pn = os.path.join(a.old, f), os.path.join(a.new, f)
        so = symbols(po) if os.path.exists(po) else {}
        sn = symbols(pn) if os.path.exists(pn) else {}
        uo, un = usage(po[:-2] + ".usage"), usage(pn[:-2] + ".usage")
        both = sorted(set(so) & set(sn))
        same = [s for s in both if so[s] == sn[s]]
        diff = [s for s in both if so[s] != sn[s]]
        added, removed = sorted(set(sn) - set(so)), sorted(set(so) - set(sn))
        usame = sum(1 for s in set(uo) & set(un) if uo[s] == un[s])
        udiff = sorted(s for s in set(uo) & set(un) if uo[s] != un[s])
        uonly = len(set(uo) ^ set(un))
        print(f"{f[:-2]}.hip: {len(same)} symbols identical, {len(diff)} differing, "
              f"{len(removed)} removed, {len(added)} added; .usage: {usame} entries identical, "
              f"{len(udiff)} differing, {uonly} unmatched")
        differs |= bool(diff or added or removed or udiff or uonly)
        nm = demangle(sorted(set(both) | set(added) | set(removed) | set(udiff)))
        for s in diff:
            what = "stream" if so[s][0] != sn[s][0] else ".amdhsa block"
            details.append(f"  {f[:-2]}.hip  {nm[s]}: {what} differs, instructions "
                           f"{_ninstr(so[s][0])} -> {_ninstr(sn[s][0])}, .usage "
                           f"{'unchanged' if uo.get(s) == un.get(s) else 'CHANGED'}")
            if uo.get(s) != un.get(s):
                details.append(f"      before: {uo.get(s)}")
                details.append(f"      after:  {un.get(s)}")
        for s in udiff:
            if s not in diff:
                details.append(f"  {f[:-2]}.hip  {nm[s]}: .usage differs: {uo[s]} -> {un[s]}")
        details += [f"  {f[:-2]}.hip  {nm[s]}: added" for s in added]
        details += [f"  {f[:-2]}.hip  {nm[s]}: removed" for s in removed]
        if a.list:
            details += [f"  {f[:-2]}.hip  {nm[s]}: identical" for s in same]
    if details:
        print()
        print("\n".join(details))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
