"""Register / spill / scratch / LDS figures and static instruction counts of the pipeline kernels from the compiler's output (no GPU
needed):
    python tools/kernel_resources.py [--src FILE]... [-D...]
compiles each FILE -- default: boundplanner_amd/csrc/bmpc_pipeline.hip and the fixed-horizon files bmpc_pair_n20.hip, bmpc_pair_n30.hip
-- for gfx950 to assembly with the product build's flags plus the given defines (~1 min per file, side by side).  `SGPR spills` is
the number of scalar registers the kernel parks in the lanes of vector registers; `instructions` counts the machine instructions
between the kernel's label and the end of its function."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(R, "boundplanner_amd", "csrc")
SRCS, DEFS, argv = [], [], sys.argv[1:]
while argv:
    a = argv.pop(0)
    if a == "--src": SRCS.append(os.path.abspath(argv.pop(0)))
    else: DEFS.append(a)
if not SRCS:
    SRCS = [os.path.join(CSRC, f) for f in ("bmpc_pipeline.hip", "bmpc_pair_n20.hip", "bmpc_pair_n30.hip") if os.path.exists(os.path.join(CSRC, f))]


def assembly(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "p.s")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", *DEFS, "--cuda-device-only", "-S",
                               src, "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()


def instructions(txt):
    """kernel symbol -> number of instruction lines of its function (labels, directives and comments are not instructions)"""
    n = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        n[m.group(1)] = sum(1 for l in m.group(2).split("\n") if re.match(r"\s+[a-z]\w*(\s|$)", l))
    return n


pat = (r"\.agpr_count:\s+(\d+).*?\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?"
       r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)")
print(f"{'kernel':28s} {'VGPRs (incl. AGPRs)':>20s} {'AGPRs':>6s} {'spilled VGPRs':>14s} {'scratch B/lane':>15s} {'static LDS B':>13s} "
      f"{'SGPR spills':>12s} {'instructions':>13s}")
with ThreadPoolExecutor(max_workers=len(SRCS)) as pool:
    for txt in pool.map(assembly, SRCS):
        count = instructions(txt)
        for ag, lds, name, priv, ssp, vg, sp in re.findall(pat, txt, re.S):
            n = re.sub(r"^_Z\d+", "", name).split("N4bmpc")[0]
            print(f"{n:28s} {vg:>20s} {ag:>6s} {sp:>14s} {priv:>15s} {lds:>13s} {ssp:>12s} {count.get(name, 0):>13d}")
