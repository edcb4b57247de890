"""Writes tests/golden/REPORT_attention_routes.txt from the figures the attention route tests append to the file
PSG_ATTN_REPORT names:  PSG_ATTN_REPORT=cpu.txt pytest tests/test_attn_ref_cpu.py;  PSG_ATTN_REPORT=gpu.txt pytest -m gpu
tests/test_attention_routes_gpu.py;  python tools/attn_routes_report.py cpu.txt gpu.txt tests/golden/REPORT_attention_routes.txt
(tests/test_attn_ref_cpu.py::test_report_states_the_constant checks the committed report against the constant in use).

python tools/attn_routes_report.py --routes  rewrites tests/golden/attn_routes.json, the expected route of every case and pass
of tests/attn_cases.py, from the library's psg_attn_route - for a deliberate routing change, to be read in the diff."""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import attn_cases as K
from tests import attn_ref as R

if sys.argv[1:2] == ["--routes"]:
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.load()
    routes = {}
    for cs in K.CASES:
        rows = []
        for p in range(len(K.PASSES)):
            rc, rt = K.query_route(lib, p, cs[1], *K.route_args(cs, p))
            assert rc == 0, (cs[0], p, rc)
            rows.append(list(rt))
        routes[cs[0]] = rows
    with open(os.path.join(ROOT, "tests", "golden", "attn_routes.json"), "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in routes.items()) + "\n}\n")
    sys.exit(0)

cpu, gpu, out = sys.argv[1:4]
FAM = {"0": "bf16 MFMA", "1": "VALU", "2": "fp32 MFMA"}
L = []
L.append("Attention route tests: the figures behind tests/attn_ref.py, tests/test_attn_ref_cpu.py and tests/test_attention_routes_gpu.py")
L.append("(written from the files the tests append to when PSG_ATTN_REPORT names one)")
L.append("")
L.append("1. The constant of the bounds")
L.append("   Smallest c at which torch's own fp32 restatement (matmul, softmax, autograd backward; bf16: inputs pre-rounded, on the")
L.append("   bf16 MFMA family P and dS rounded to bf16, outputs rounded to bf16) passes each bound against the fp64 reference: the")
L.append(f"   largest over the {len(K.CASES)} cases x 2 launch pairs (plain, key lengths).")
cm = {}
for l in open(cpu):
    f = l.split()
    if f[0] == "torch_c_max": cm[(f[1], f[2])] = float(f[3])
L.append("   output    fp32      bf16")
for o in R.OUTPUTS:
    L.append(f"   {o:<8} {cm[('f32', o)]:<9.4g} {cm[('bf16', o)]:<9.4g}")
top = max(cm.values())
L.append(f"   largest: {top:.4g} -> C_TORCH = {R.C_TORCH:g}, C_ATTN = 4 x C_TORCH = {R.C_ATTN:g} (one value for all outputs)")
L.append("   The constant is fixed in tests/attn_ref.py so that every host holds the kernels to one bound; the CPU test requires")
L.append("   this measurement to lie within [0.8, 1] x C_TORCH on the host it runs on.")
L.append("   (0: the error fits the output's own rounding and the analytic extra terms alone)")
L.append("")
L.append("2. The formula model (fp32, P from the stored lse, delta as the kernels form it; bf16 MFMA: P and dS rounded to bf16):")
L.append("   largest fraction of the bound at C_ATTN used, per dtype and family (CPU)")
mo = collections.defaultdict(lambda: collections.defaultdict(float))
for l in open(cpu):
    f = l.split()
    if f[0] == "model":
        for kv in f[4:]:
            k, v = kv.split("="); mo[(f[2], f[3])][k] = max(mo[(f[2], f[3])][k], float(v))
for (d, fam), m in sorted(mo.items()):
    L.append(f"   {d:<5} {FAM[fam[-1]]:<10} " + " ".join(f"{k}={v:.3g}" for k, v in m.items()))
L.append("")
L.append("3. Which output caught each defect (launches on which the defect was injected: caught by that output / all)")
mu = collections.defaultdict(lambda: collections.Counter())
tot = collections.Counter()
for l in open(cpu):
    f = l.split()
    if f[0] == "mutation":
        tot[f[1]] += 1
        for o in f[6].split(","): mu[f[1]][o] += 1
for m in sorted(tot):
    L.append(f"   {m:<21} {tot[m]:>3} launches: " + ", ".join(f"{o} {n}" for o, n in sorted(mu[m].items(), key=lambda t: -t[1])))
missed = sum(c["NONE"] for c in mu.values())
L.append("   No launch left a defect uncaught." if not missed else f"   {missed} LAUNCHES LEFT A DEFECT UNCAUGHT (NONE above).")
L.append("")
L.append("4. MI355X: largest fraction of its bound each output used, per dtype and family (never used to tune the bound)")
g = collections.defaultdict(lambda: collections.defaultdict(float))
where = {}
n = 0
for l in open(gpu):
    f = l.split()
    if f[0] != "gpu": continue
    n += 1
    for kv in f[5:]:
        k, v = kv.split("=")
        key = (f[2], f[4])
        if float(v) >= g[key][k]:
            g[key][k] = float(v); where[key + (k,)] = f"{f[1]} {f[3]}"
for key, m in sorted(g.items()):
    L.append(f"   {key[0]:<5} {FAM[key[1][-1]]:<10} " + " ".join(f"{k}={v:.3g}" for k, v in m.items()))
L.append(f"   ({n} launches; every element of every output within its bound)" if n else "   (no MI355X figures in this run)")
L.append("")
L.append("5. The loosest check")
if g:
    lo = min(((v, key, k) for key, m in g.items() for k, v in m.items() if k in m), key=lambda t: t[0])
    L.append(f"   The output whose kernels use the least of their bound: {lo[2]} on {lo[1][0]} {FAM[lo[1][1][-1]]}, at most {lo[0]:.3g} of it")
    L.append(f"   (largest at {where[lo[1] + (lo[2],)]}): a defect there must be that much larger than the kernels' own error to be seen.")
L.append("   By construction the loosest check is the one whose bound is mostly absolute terms: on the bf16 MFMA family the")
L.append("   worst-case sum of the 2^-8 roundings of P and dS (they add like a random walk, the bound adds their magnitudes), and")
L.append("   c_acc, which is floored at 32 x 2^-24 and multiplies the score error of every head_dim below 1024.")
open(out, "w").write("\n".join(L) + "\n")
print("\n".join(L))
if missed:
    sys.exit(f"{missed} launches left a defect uncaught")
