"""device code of two source trees compared kernel by kernel (hipcc --cuda-device-only -S with the flags of
__graft_entry__.build_hip, no GPU needed): python tools/isa_identity.py [--removed-ok] BEFORE_TREE AFTER_TREE
Each tree's symbols are the union over its csrc/*.hip units, so a kernel may move between units; a kernel that two units
of one tree define is an error.  Prints every function symbol whose instruction lines or .amdhsa_* directives differ, or
that one tree alone has, and exits 1 if there is any: the gate of a host-side refactor (identical code objects have no
speed to measure).  --removed-ok: symbols that only BEFORE has are listed under their own heading and do not fail the run
(deleting dead kernels); symbols that only AFTER has, and differing symbols, always fail."""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as g  # noqa: E402


def extra_flags(src):
    """the per-file flags of __graft_entry__.build_hip -- keep the two rules the same"""
    base = os.path.basename(src)
    if base.startswith("solver_") or base == "vis.hip":
        return ["-ffp-contract=off"]
    return []


def device_asm(src):
    with tempfile.NamedTemporaryFile(suffix=".s") as out:
        r = subprocess.run([g.HIPCC] + g.HIP_FLAGS + extra_flags(src) + ["--cuda-device-only", "-S", src, "-o", out.name],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("%s does not compile:\n%s" % (src, r.stderr[-3000:]))
        return open(out.name).read()


def symbols(asm):
    """{symbol: its instruction, label and .amdhsa_* lines} (block labels without the function's running number)"""
    syms, cur = {}, None
    for line in asm.splitlines():
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        if not line or "__hip_cuid_" in line:
            continue
        m = re.match(r"\.type\s+(\S+),@function|\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = syms.setdefault(m.group(1) or m.group(2), [])
        elif re.match(r"\.Lfunc_end\d+:|\.end_amdhsa_kernel", line):
            cur = None
        elif cur is not None and (not line.startswith(".") or line.startswith((".amdhsa_", ".LBB_"))):
            cur.append(line)
    return syms


def tree_symbols(tree, ex, pattern="*.hip"):
    """({symbol: [(unit, lines), ...]}, [kernels that two units define]) over the tree's units.  A device function that
    is not a kernel stays inside its unit's code object (the build has no relocatable device code), so two units may each
    hold their own copy of one (sm::jacobi_svd); every copy is kept and compared."""
    srcs = sorted(glob.glob(os.path.join(tree, "df-vo_amd", "csrc", pattern)))
    syms, twice = {}, []
    for src, asm in zip(srcs, ex.map(device_asm, srcs)):
        kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
        for s, lines in symbols(asm).items():
            if s in kernels and s in syms:
                twice.append("%s: %s and %s" % (s, syms[s][0][0], os.path.basename(src)))
            syms.setdefault(s, []).append((os.path.basename(src), lines))
    return syms, twice


def main(before, after, removed_ok=False, pattern="*.hip"):
    with ThreadPoolExecutor(max_workers=8) as ex:
        (a, twice_a), (b, twice_b) = tree_symbols(before, ex, pattern), tree_symbols(after, ex, pattern)
    for tree, twice in ((before, twice_a), (after, twice_b)):
        for t in twice:
            print("kernel defined twice in %s: %s" % (tree, t))
    units = lambda copies: ", ".join(u for u, _ in copies)
    bodies = lambda copies: sorted(lines for _, lines in copies)
    differs = sorted(s for s in a.keys() & b.keys() if bodies(a[s]) != bodies(b[s]))
    removed, added = sorted(a.keys() - b.keys()), sorted(b.keys() - a.keys())
    for s in differs:
        print("%s -> %s: %s differs" % (units(a[s]), units(b[s]), s))
    for s in added:
        print("%s: %s only in %s" % (units(b[s]), s, after))
    if removed:
        print("removed (only in %s)%s:" % (before, ", allowed by --removed-ok" if removed_ok else ""))
        for s in removed:
            print("  %s: %s" % (units(a[s]), s))
    bad = len(differs) + len(added) + len(twice_a) + len(twice_b) + (0 if removed_ok else len(removed))
    print("%d of %d symbols differ, %d only in AFTER, %d removed, %d kernels defined twice" %
          (len(differs), len(a.keys() | b.keys()), len(added), len(removed), len(twice_a) + len(twice_b)))
    return 1 if bad else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--removed-ok"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], removed_ok="--removed-ok" in sys.argv[1:]))
