"""Writes tests/golden/REPORT_groupnorm_routes.txt from the figures the GroupNorm route tests append to the file PSG_GN_REPORT
names:  PSG_GN_REPORT=cpu.txt pytest tests/test_gn_ref_cpu.py;  PSG_GN_REPORT=gpu.txt pytest -m gpu
tests/test_groupnorm_routes_gpu.py;  python tools/gn_routes_report.py cpu.txt gpu.txt tests/golden/REPORT_groupnorm_routes.txt
(tests/test_gn_ref_cpu.py::test_report_states_the_constant checks the committed report against the constant in use)."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import gn_ref as R

cpu, gpu, out = sys.argv[1:4]
L = []
L.append("GroupNorm route tests: the figures behind tests/gn_ref.py, tests/test_gn_ref_cpu.py and tests/test_groupnorm_routes_gpu.py")
L.append("(written from the files the tests append to when PSG_GN_REPORT names one)")
L.append("")
L.append("1. The constant of the bounds")
L.append("   Smallest c at which torch's own fp32 F.group_norm (+ F.silu, autograd backward; bf16: inputs pre-rounded, y and dx")
L.append("   rounded to bf16) passes each bound against the fp64 reference: the largest over the 18 cases x 2 variants.")
cm = {}
for l in open(cpu):
    f = l.split()
    if f[0] == "torch_c_max": cm[(f[1], f[2])] = float(f[3])
L.append("   output    fp32      bf16")
for o in ("y","mean","rstd","dx","dgamma","dbeta"):
    L.append(f"   {o:<8} {cm[('f32',o)]:<9.4g} {cm[('bf16',o)]:<9.4g}")
top = max(cm.values())
L.append(f"   largest: {top:.4g} -> C_TORCH = {R.C_TORCH:g}, C_GN = 4 x C_TORCH = {R.C_GN:g} (one value for all outputs)")
L.append("   The constant is fixed in tests/gn_ref.py so that every host holds the kernels to one bound; the CPU test requires")
L.append("   this measurement to lie within [0.8, 1] x C_TORCH on the host it runs on (torch's CPU summation order depends on")
L.append("   vector width and thread count), so the margin over a host's own figure is 4x to 5x.")
L.append("   (0: the error fits the output's own rounding and, for dx, the c_acc reduction terms alone)")
L.append("   Known weak spot: dx.  Its reduction terms rstd (e1 + xa e2), e = c_acc(n) mean_g|terms|, are absolute terms that")
L.append("   stand outside C_GN, and c_acc is floored at 32 x 2^-24, so they dominate the fp32 dx bound: torch needs")
fdx = max([float(kv.split("=")[1]) for l in open(gpu) for kv in l.split() if l.startswith("gpu ") and " f32 " in l and kv.startswith("dx=")] or [float("nan")])
L.append(f"   c = {cm[('f32', 'dx')]:.3g} and the fp32 kernels use at most {fdx:.3g} of it (section 4): the fp32 dx check is that much looser than the y check.")
L.append("")
L.append("2. fp32 emulation of the split forward's summation order: largest fraction of the bound used (CPU)")
se = collections.defaultdict(lambda: collections.defaultdict(float))
for l in open(cpu):
    f = l.split()
    if f[0] == "split_emulation":
        kind = f[3] if f[3] == "const" else "table"
        for kv in f[4:]:
            k, v = kv.split("="); se[(f[2], kind)][k] = max(se[(f[2], kind)][k], float(v))
for (d, kind), m in sorted(se.items()):
    L.append(f"   {d:<5} {kind:<6} " + " ".join(f"{k}={v:.3g}" for k, v in m.items()))
L.append("   table: every launch whose forward is split, (5, 2000, 64, 32) on x = 4 + 0.75 u among them; const: sample 1 constant.")
L.append("   The emulation adds the PP x Cg lane sums of gn_stats_kernel in double, as the kernel does.  Recorded once, not")
L.append("   regenerated: with those sums added in fp32 the emulation missed the fp32 y bound on that input by a factor 1.4.")
L.append("   The split backward's order is not emulated.")
L.append("")
L.append("3. Which output caught each defect (launches on which the defect applies: caught by that output / all)")
mu = collections.defaultdict(lambda: collections.Counter())
tot = collections.Counter()
for l in open(cpu):
    f = l.split()
    if f[0] == "mutation":
        tot[f[1]] += 1
        for o in f[6].split(","): mu[f[1]][o] += 1
for m in ("stat_last_pixel","count_padded","straddle","dres_column","last_split","sample32","silu_no_beta","no_accumulate","no_gamma_in_sums"):
    L.append(f"   {m:<17} {tot[m]:>3} launches: " + ", ".join(f"{o} {n}" for o, n in sorted(mu[m].items(), key=lambda t: -t[1])))
missed = sum(c["NONE"] for c in mu.values())
L.append("   No launch left a defect uncaught." if not missed else f"   {missed} LAUNCHES LEFT A DEFECT UNCAUGHT (NONE above).")
L.append("")
L.append("4. MI355X: largest fraction of its bound each output used, per route (dtype direction route: output=fraction)")
g = collections.defaultdict(lambda: collections.defaultdict(float))
n = 0
for l in open(gpu):
    f = l.split()
    if f[0] != "gpu": continue
    n += 1
    d = f[2]
    routes = {r.split(":")[0]: r.split(":")[1] for r in f[4:] if r.startswith(("fwd:","bwd:"))}
    for kv in f[4:]:
        if "=" not in kv: continue
        k, v = kv.split("=")
        direction = "fwd" if k in ("y","mean","rstd") else "bwd"
        rt = routes[direction]
        g[(d, direction, rt)][k] = max(g[(d, direction, rt)][k], float(v))
for key, m in sorted(g.items()):
    L.append(f"   {key[0]:<5} {key[1]} {key[2]:<20} " + " ".join(f"{k}={v:.3g}" for k, v in m.items()))
L.append(f"   ({n} forward + backward launch pairs and extra forwards; every element of every output within its bound)")
open(out, "w").write("\n".join(L) + "\n")
print("\n".join(L))
if missed:
    sys.exit(f"{missed} launches left a defect uncaught")
