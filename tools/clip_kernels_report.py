"""Writes tests/golden/REPORT_clip_kernels.txt from the figures the element-wise CLIP kernel tests append to the file
PSG_CLIP_REPORT names:
PSG_CLIP_REPORT=cpu.txt pytest tests/test_clip_ref_cpu.py;  PSG_CLIP_REPORT=gpu.txt pytest -m gpu tests/test_clip_kernels_gpu.py;
python tools/clip_kernels_report.py cpu.txt gpu.txt tests/golden/REPORT_clip_kernels.txt [conv_gpu.txt]
(conv_gpu.txt: the PSG_CONV_REPORT file of a GPU run of tests/test_conv_routes_gpu.py, for the quick-GELU cases)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import clip_cases as K
from tests import clip_ref as R
from tests import conv_cases

cpu, gpu, out = sys.argv[1:4]
conv = sys.argv[4] if len(sys.argv) > 4 else None
cpu_lines = [l.strip() for l in open(cpu)]
L = ["CLIP kernels (csrc/clip.hip) and the quick-GELU epilogue, element by element: the figures behind tests/clip_cases.py,",
     "tests/test_clip_ref_cpu.py and tests/test_clip_kernels_gpu.py (written from the files the tests append to when",
     "PSG_CLIP_REPORT names one)", ""]
L.append("1. The constants of the bounds (measured on the CPU, never against a kernel)")
for l in cpu_lines:
    if l.startswith(("c_causal", "c_cos", "prep_f32")):
        L.append("   " + l)
L.append(f"   C_CAUSAL = 4 x max({R.C_CAUSAL_TORCH}, {R.C_CAUSAL_SEQ}) = {R.C_CAUSAL:.4g};  C_COS = 4 x {R.C_COS_TORCH} = {R.C_COS:.4g};  K_PREP = {R.K_PREP} (counted)")
L.append("   The recorded values are fixed in tests/clip_ref.py so that every host holds the kernels to one bound; the CPU tests")
L.append("   require a re-measurement within 25 %.")
L.append("")
L.append(f"2. The table: {len(K.CAUSAL)} causal cases, {len(K.PREP_SHAPES) * len(K.PREP_BATCHES) * len(K.DTYPES)} prep cases x {len(K.PREP_AB)} (a, b) x "
         f"{len(K.PREP_LD_EXTRA)} row strides, {len(K.COS_B) * len(K.COS_D) * len(K.DTYPES)} cosine cases x up to {len(K.COS_KINDS)} row kinds")
L.append("")
L.append("3. Planted defects (fp64 emulation at the table's shapes): kernel, defect, the smallest case, which rejected it")
for l in cpu_lines:
    if l.startswith("defect "):
        L.append("   " + l[len("defect "):])
L.append("")
L.append("4. The kernels on an MI355X: worst |err| / bound per case and output (0 = a bit comparison: a bf16 prep forward is the fp32")
L.append("   launch's result rounded to nearest even)")
worst = {}
for l in open(gpu):
    f = l.split()
    if not f or f[0] != "gpu":
        continue
    L.append("   " + l.strip()[4:])
    dn = "bf16" if "bf16" in l else "f32"
    for kv in f[2:]:
        if "=" in kv:
            k, v = kv.split("=")
            key = (f[1], dn, k)
            if key not in worst or float(v) > worst[key][0]:
                worst[key] = (float(v), " ".join(x for x in f[2:] if "=" not in x))
L.append("   largest per kernel, dtype and output (never used to tune a bound):")
for (kern, dn, k), (v, case) in sorted(worst.items()):
    L.append(f"   {kern:<7} {dn:<5} {k:<5} {v:<8.3g} {case}")
L.append("   A bf16 value near 1 is the output's own rounding: 2^-8 |ref| is half an ulp, all of which a correctly rounded result may use.")
if conv:
    L.append("")
    L.append("5. Quick-GELU on the conv epilogue paths (tests/conv_cases.py, section H; gemm_ref.check): case, epilogue form, worst err / bound")
    for l in open(conv):
        r = json.loads(l)
        if "case" in r and conv_cases.BY_NAME[r["case"]]["act"] == "quick_gelu":
            L.append(f"   {r['case']:<38} {','.join(sorted(set(r['forms']))):<24} " + " ".join(f"{k}={v:.3g}" for k, v in r["ratios"].items()))
with open(out, "w") as f:
    f.write("\n".join(L) + "\n")
