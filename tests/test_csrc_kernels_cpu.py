"""CPU: no dead kernels in csrc.  A text scan, nothing is compiled: every `__global__` function defined in csrc/*.hip and
csrc/*.h must be named, outside comments, at least once more in csrc besides its own declarations -- by a launch, an
ensure_dyn_lds cast or an explicit instantiation.  A kernel that a fused one replaced and nobody launches costs every
reader of its file, and the comments of its successors keep leaning on it."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "df-vo_amd", "csrc")
COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)
KERNEL_DECL = re.compile(r"__global__\b[^;{()]*(?:__launch_bounds__\s*\([^;{]*?\)\s*)?void\s+(\w+)\s*\(")


def unreferenced_kernels(texts):
    """names of the kernels that `texts` (comment-free sources) declare and never name again"""
    code = "\n".join(texts)
    declared = KERNEL_DECL.findall(code)
    return sorted(k for k in set(declared) if len(re.findall(r"\b%s\b" % k, code)) <= declared.count(k))


def test_scanner_sees_a_dead_kernel_and_only_that():
    live = "template <int N> __global__ __launch_bounds__(64 * N, 2) void k_live(int* p) {}\nvoid f() { k_live<2><<<1, 128>>>(0); }"
    dead = "// k_dead is launched nowhere\n__global__ void k_dead(int* p) { /* k_dead */ }"
    assert unreferenced_kernels([COMMENT.sub("", live), COMMENT.sub("", dead)]) == ["k_dead"]


def test_every_kernel_is_referenced():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    texts = [COMMENT.sub("", open(p).read()) for p in paths]
    assert sum(len(KERNEL_DECL.findall(t)) for t in texts) > 50, "the scan no longer recognises the kernels"
    dead = unreferenced_kernels(texts)
    assert not dead, "kernels that nothing launches: " + ", ".join(dead)
