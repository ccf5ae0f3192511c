#!/usr/bin/env python3
"""Did a source change move a kernel's instructions?  Compiles .hip units of
two source trees to gfx950 assembly with the library's own flags
(s3dlio_amd/build.py: compile_flags, plus --cuda-device-only -S and the
compiler's resource-usage remarks) and compares, kernel symbol by kernel
symbol, the instruction streams: the assembly text of each kernel with
comments, directives and labels removed (local labels keep their number
within the function, not the function's index in its unit).

    python tools/kernel_streams.py --a OLD_ROOT s3dg_kernels.hip \\
                                   --b . s3dg_block.hip s3dg_ks_kernels.hip

A root is a checkout (include/ and s3dlio_amd/csrc/ below it); units are names
in its csrc.  A tree's units may differ: the symbols of all of them are pooled.
Reported: symbols in one tree only; the number of identical streams; for each
changed symbol both instruction counts and whether the two streams are the
same multiset of lines (instructions reordered, none added or dropped); the
symbols whose resource usage (SGPRs, VGPRs, AGPRs, scratch, occupancy, spills,
LDS) differs.  Exit status 1 when the symbol sets differ.

Text comparison only, no GPU.  One hipcc per unit, MAX_JOBS at a time
(default: the CPUs, at most 16).
Tooling only: nothing in the product imports this."""
import argparse, collections, concurrent.futures as cf, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s3dlio_amd"))
import build as B   # by path: importing the package would load the library


def compile_unit(root, unit, out):
    """(assembly text, remarks text) of one unit of the tree at root."""
    src = os.path.join(root, "s3dlio_amd", "csrc", unit)
    cmd = [B.HIPCC, *B.compile_flags(root), "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           "-o", out, src]
    p = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        sys.exit(f"{' '.join(cmd)}\n{p.stderr[-4000:]}")
    with open(out) as f:
        return f.read(), p.stderr


def streams(asm):
    """{kernel symbol: [instruction line, ...]}."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur = {}, None
    for line in asm.splitlines():
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        if line.endswith(":"):
            if line[:-1] in kernels:
                cur = out.setdefault(line[:-1], [])
            elif line.startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None or line.startswith("."):
            continue
        cur.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", " ".join(line.split())))
    assert set(out) == kernels, sorted(kernels ^ set(out))
    return out


def resources(remarks):
    """{symbol: {figure: value}} from the resource-usage remarks."""
    out, cur = {}, None
    for m in re.finditer(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", remarks):
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return out


def pooled(units, futs):
    """The streams and resource figures of a tree's units together."""
    S, R = {}, {}
    for u, f in zip(units, futs):
        asm, remarks = f.result()
        s = streams(asm)
        assert not set(s) & set(S), f"{u}: a kernel symbol of another unit"
        S.update(s)
        R.update({k: v for k, v in resources(remarks).items() if k in s})
    return S, R


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--a", nargs="+", required=True, metavar=("ROOT", "UNIT"))
    ap.add_argument("--b", nargs="+", required=True, metavar=("ROOT", "UNIT"))
    args = ap.parse_args()
    if len(args.a) < 2 or len(args.b) < 2:
        ap.error("each tree is a root and at least one unit")
    jobs = int(os.environ.get("MAX_JOBS", "0")) or min(16, os.cpu_count() or 1)
    with tempfile.TemporaryDirectory(prefix="kstreams_") as tmp, cf.ThreadPoolExecutor(jobs) as pool:
        fa, fb = ([pool.submit(compile_unit, os.path.abspath(t[0]), u, os.path.join(tmp, f"{tag}_{u}.s"))
                   for u in t[1:]] for tag, t in (("a", args.a), ("b", args.b)))
        (SA, RA), (SB, RB) = pooled(args.a[1:], fa), pooled(args.b[1:], fb)
    print(f"a: {' '.join(args.a[1:])}: {len(SA)} kernel symbols")
    print(f"b: {' '.join(args.b[1:])}: {len(SB)} kernel symbols")
    for tag, only in (("a", sorted(set(SA) - set(SB))), ("b", sorted(set(SB) - set(SA)))):
        print(f"only in {tag}: {len(only)}")
        for k in only:
            print(f"  {k}")
    both = sorted(set(SA) & set(SB))
    changed = [k for k in both if SA[k] != SB[k]]
    print(f"identical streams: {len(both) - len(changed)} of {len(both)}")
    print(f"changed streams: {len(changed)}")
    for k in changed:
        same = collections.Counter(SA[k]) == collections.Counter(SB[k])
        print(f"  {k}: {len(SA[k])} -> {len(SB[k])} instructions, "
              f"{'the same multiset of lines' if same else 'different lines'}")
    res = [k for k in both if RA.get(k) != RB.get(k)]
    print(f"resource usage: {len(both) - len(res)} of {len(both)} unchanged "
          f"({', '.join(sorted(next(iter(RA.values()))))})" if RA else "resource usage: no remarks")
    for k in res:
        diff = {f: (RA.get(k, {}).get(f), RB.get(k, {}).get(f))
                for f in sorted(set(RA.get(k, {})) | set(RB.get(k, {}))) if RA.get(k, {}).get(f) != RB.get(k, {}).get(f)}
        print(f"  {k}: " + ", ".join(f"{f} {a} -> {b}" for f, (a, b) in diff.items()))
    sys.exit(1 if set(SA) != set(SB) else 0)


if __name__ == "__main__":
    main()
