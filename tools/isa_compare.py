#!/usr/bin/env python3
"""Compares two builds of one kernel family kernel by kernel (no GPU needed): the resource figures of hipcc's
-Rpass-analysis=kernel-resource-usage remarks and the instruction streams of the two assembly files.

  make -C g.p.u-pathtracer_amd isa K=pt_k_wave 2> wave.remarks && cp /tmp/pt_k_wave.gfx950.s wave.s      (at both commits)
  tools/isa_compare.py parent/wave.remarks parent/wave.s head/wave.remarks head/wave.s [--rename OLD=NEW ...]

--rename OLD=NEW (mangled names, repeatable): the parent's kernel OLD is compared with the head's NEW — for a kernel whose
name changed but whose code must not have, such as one that gained a template argument.

A stream is a kernel's lines without comments, directives and blank lines, every local label (.LBBn_m) renamed to one token.
Prints one line per kernel: VGPRs, then occupancy / scratch / SGPR spill / VGPR spill / LDS on both sides, the instruction
counts, and whether the streams are identical; where they are not, the first instruction at which they part.  Exit status 1
when the sets of kernels or any resource figure differ.

  tools/isa_compare.py parent/wave.remarks parent/wave.s head/wave.remarks head/wave.s --by-content

--by-content: for a change that renames every kernel (other template arguments) and must change no code.  The two builds are compared as
multisets of (family = the demangled name in front of `<`, instruction stream, all resource figures, VGPRs included).  A stream
does not contain its kernel's own name; a call of another function would, and these kernels have none.  Prints per family the
number of kernels on each side and how many have no partner on the other.  Exit status 1 on any difference."""
import collections
import re
import subprocess
import sys

FIELDS = ("VGPRs", "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def resources(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    return out


def streams(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"([A-Za-z_]\w*):\s", line)   # mangled, or extern "C"
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") and not s.startswith(".LBB"):
            continue
        s = re.sub(r"\.LBB\d+_\d+", ".L", s)
        if s != ".L:":
            cur.append(s)
    return out


def demangle(names):
    text = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout
    return dict(zip(names, (t.replace("void ", "").replace("(KParams)", "") for t in text.splitlines())))


def by_content(ra, sa, rb, sb):
    """The two builds as multisets of (instruction stream, resource figures), whatever the kernels are called."""
    def family(pretty):
        return re.match(r"(?:\(anonymous namespace\)::)?[^<(]*", pretty).group(0)

    def bag(res, strm):
        pretty, out = demangle(sorted(res)), collections.Counter()
        for n in res:
            out[(family(pretty[n]), tuple(strm[n]), tuple(res[n].get(f) for f in FIELDS))] += 1
        return out
    a, b = bag(ra, sa), bag(rb, sb)
    bad = False
    print("family | kernels parent -> head | without a partner: parent, head")
    for fam in sorted({k[0] for k in a} | {k[0] for k in b}):
        na, nb = sum(c for k, c in a.items() if k[0] == fam), sum(c for k, c in b.items() if k[0] == fam)
        la, lb = sum(c for k, c in (a - b).items() if k[0] == fam), sum(c for k, c in (b - a).items() if k[0] == fam)
        bad |= na != nb or la != 0 or lb != 0
        print(f"{fam} | {na} -> {nb} | {la}, {lb}")
    print(f"total | {sum(a.values())} -> {sum(b.values())} | {sum((a - b).values())}, {sum((b - a).values())} | {'DIFFERENT' if bad else 'identical'}")
    return 1 if bad else 0


def main():
    ra, sa, rb, sb = resources(sys.argv[1]), streams(sys.argv[2]), resources(sys.argv[3]), streams(sys.argv[4])
    if sys.argv[5:] == ["--by-content"]:
        return by_content(ra, sa, rb, sb)
    for k in range(5, len(sys.argv) - 1, 2):
        assert sys.argv[k] == "--rename", sys.argv[k]
        old, new = sys.argv[k + 1].split("=")
        ra[new], sa[new] = ra.pop(old), sa.pop(old)
    names = sorted(set(ra) | set(rb))
    pretty = demangle(names)
    bad = False
    print("kernel | VGPRs | occupancy scratch sgpr-spill vgpr-spill lds (parent -> head) | instructions | stream")
    for n in names:
        if n not in ra or n not in rb:
            print(f"{pretty[n]} | only in {'parent' if n in ra else 'head'}")
            bad = True
            continue
        a, b = [ra[n].get(f) for f in FIELDS], [rb[n].get(f) for f in FIELDS]
        bad |= a[1:] != b[1:]
        same = sa[n] == sb[n]
        where = ""
        if not same:
            k = next((i for i, (x, y) in enumerate(zip(sa[n], sb[n])) if x != y), min(len(sa[n]), len(sb[n])))
            where = f" (part at instruction {k}: `{sa[n][k] if k < len(sa[n]) else 'end'}` / `{sb[n][k] if k < len(sb[n]) else 'end'}`)"
        fig = " ".join(map(str, a[1:])) + (" = same" if a[1:] == b[1:] else " -> " + " ".join(map(str, b[1:])))
        print(f"{pretty[n]} | {a[0]} -> {b[0]} | {fig} | {len(sa[n])} -> {len(sb[n])} | {'identical' if same else 'DIFFERENT' + where}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
