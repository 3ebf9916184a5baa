"""device code of two source trees compared kernel by kernel (hipcc --cuda-device-only -S with the flags of
__graft_entry__.build_hip, no GPU needed): python tools/isa_identity.py BEFORE_TREE AFTER_TREE
Prints every function symbol whose instruction lines or .amdhsa_* directives differ, or that one tree alone has, and
exits 1 if there is any: the gate of a host-side refactor (identical code objects have no speed to measure)."""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as g  # noqa: E402


def device_asm(src):
    extra = ["-ffp-contract=off"] if os.path.basename(src).startswith("solver_") else []
    with tempfile.NamedTemporaryFile(suffix=".s") as out:
        r = subprocess.run([g.HIPCC] + g.HIP_FLAGS + extra + ["--cuda-device-only", "-S", src, "-o", out.name],
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


def main(before, after):
    units = sorted({os.path.basename(s) for t in (before, after) for s in glob.glob(os.path.join(t, "df-vo_amd", "csrc", "*.hip"))})
    paths = [os.path.join(t, "df-vo_amd", "csrc", u) for u in units for t in (before, after)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        asm = dict(zip(paths, ex.map(lambda s: symbols(device_asm(s)) if os.path.exists(s) else {}, paths)))
    bad = total = 0
    for u in units:
        a, b = (asm[os.path.join(t, "df-vo_amd", "csrc", u)] for t in (before, after))
        total += len(a.keys() | b.keys())
        for s in sorted(a.keys() | b.keys()):
            if a.get(s) != b.get(s):
                bad += 1
                print("%s: %s %s" % (u, s, "differs" if s in a and s in b else "only in " + (before if s in a else after)))
    print("%d of %d symbols differ" % (bad, total))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
