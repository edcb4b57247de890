"""Writes tests/golden/REPORT_attn_longq.txt from the figures the long-query attention tests append to the file
PSG_ATTN_LONGQ_REPORT names:  PSG_ATTN_LONGQ_REPORT=cpu.txt pytest tests/test_attn_longq_ref_cpu.py;
PSG_ATTN_LONGQ_REPORT=gpu.txt pytest -m gpu tests/test_attn_longq_gpu.py;
python tools/attn_longq_report.py cpu.txt gpu.txt tests/golden/REPORT_attn_longq.txt
(tests/test_attn_longq_ref_cpu.py::test_report_states_the_constants checks the committed report against the constants in use)."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import attn_longq_cases as K
from tests import attn_ref as R

cpu, gpu, out = sys.argv[1:4]
cpu = [l.split() for l in open(cpu)]
gpu = [l.rstrip("\n") for l in open(gpu) if l.startswith("gpu")]
NAMES = ("delta", "dq", "dk", "dv")
L = []
L.append("Long-query attention backward (psg_attn_bwd_longq): the figures behind tests/attn_longq_cases.py,")
L.append("tests/test_attn_longq_ref_cpu.py and tests/test_attn_longq_gpu.py (written from the files the tests append to when")
L.append("PSG_ATTN_LONGQ_REPORT names one)")
L.append("")
L.append("1. The constant of the bounds")
L.append("   Smallest c at which torch's own fp32 restatement (matmul, softmax, autograd backward; bf16: inputs pre-rounded, outputs")
L.append(f"   rounded to bf16) passes each bound of tests/attn_ref.py against the fp64 reference: the largest over the {len(K.CASES)} cases of")
L.append("   the table, and the case it was measured on.  Measured against torch on the CPU, never against the kernel.")
cm = {(f[1], f[2]): (float(f[3]), f[4]) for f in cpu if f[0] == "torch_c_max"}
L.append(f"   {'output':<9} {'fp32':<41} bf16")
for o in R.OUTPUTS:
    cell = lambda c, where: f"{c:<9.4g} {where if c else ''}"
    L.append(f"   {o:<9} {cell(*cm[('f32', o)]):<41} {cell(*cm[('bf16', o)])}".rstrip())
top = max(c for c, _ in cm.values())
L.append(f"   largest: {top:.4g} -> C_TORCH_LONGQ = {K.C_TORCH_LONGQ:g}, C_LONGQ = 4 x max(C_TORCH, C_TORCH_LONGQ) = {K.C_LONGQ:g}")
L.append(f"   (C_TORCH = {R.C_TORCH:g}: the same measurement on the table of tests/attn_cases.py, tests/golden/REPORT_attention_routes.txt)")
L.append("   The constant is fixed in tests/attn_longq_cases.py so that every host holds the kernel to one bound; the CPU test")
L.append("   requires this measurement to lie within [0.8, 1] x C_TORCH_LONGQ on the host it runs on.")
L.append("   (0: the error fits the output's own rounding and the analytic extra terms alone)")
L.append("")
L.append("2. The formula model of the kernel pair (fp32 torch on the CPU; P from the stored lse, delta from the stored o):")
L.append("   largest fraction of the bound at C_LONGQ used, per dtype")
mo = collections.defaultdict(lambda: collections.defaultdict(float))
for f in cpu:
    if f[0] == "model":
        for kv in f[3:]:
            k, v = kv.split("="); mo[f[2]][k] = max(mo[f[2]][k], float(v))
for d in K.DTYPES:
    L.append(f"   {d:<5} " + " ".join(f"{k}={mo[d][k]:.3g}" for k in NAMES))
L.append("")
L.append("3. Which outputs caught each planted defect (case: the outputs out of bound at C_LONGQ)")
missed = 0
for f in cpu:
    if f[0] == "mutation":
        L.append(f"   {f[1]:<22} {f[2]:<28} {f[4]}")
        missed += f[4] == "NONE"
L.append("   No case left a defect uncaught." if not missed else f"   {missed} CASES LEFT A DEFECT UNCAUGHT (NONE above).")
L.append("")
L.append("4. The kernel on an MI355X: worst |err| / bound per output at C_LONGQ of every case (its layout, query tiles per slab, slabs,")
L.append("   key tiles), then the launches on psg_attn_fwd's own o and lse (gpu-fwd-pair) and through ops.attention_cross_longq (gpu-ops)")
g = collections.defaultdict(dict)
for l in gpu:
    L.append("   " + l)
    f = l.split()
    if f[0] != "gpu":
        continue
    d = [c.dname for c in K.CASES if c.name == f[1]][0]
    for kv in f[6:]:
        k, v = kv.split("=")
        if float(v) >= g[d].get(k, (0.0, ""))[0]:
            g[d][k] = (float(v), f[1])
L.append("   largest per dtype and output (never used to tune the bound):")
for d in K.DTYPES:
    if d in g:
        L.append(f"   {d:<5} " + "  ".join(f"{k}={g[d][k][0]:.3g} ({g[d][k][1]})" for k in NAMES))
L.append("   A bf16 value near 1 is the output's own rounding: 2^-8 |ref| is half an ulp, all of which a correctly rounded result")
L.append("   may use (the CPU model of section 2 uses as much); the fp32 launches show what the summation order costs.")
open(out, "w").write("\n".join(L) + "\n")
print("\n".join(L))
if missed:
    sys.exit(f"{missed} cases left a defect uncaught")
