"""Writes tests/golden/REPORT_text_rows.txt from the figures the text-encoder row-kernel tests append to the file PSG_LN_REPORT
names:  PSG_LN_REPORT=cpu.txt pytest tests/test_ln_ref_cpu.py;  PSG_LN_REPORT=gpu.txt pytest -m gpu tests/test_ln_kernels_gpu.py;
python tools/text_rows_report.py cpu.txt gpu.txt tests/golden/REPORT_text_rows.txt
(tests/test_ln_ref_cpu.py::test_report_states_the_constant checks the committed report against the constant in use)."""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ln_cases as K
from tests import ln_ref as R

cpu, gpu, out = sys.argv[1:4]
rows = [l.split() for l in open(cpu) if l.strip()]
L = []
L.append("Text-encoder row kernels (psg_layernorm, psg_layernorm_bwd, psg_bert_embed_ln, psg_bert_embed_ln_bwd, psg_embed_scatter):")
L.append("the figures behind tests/ln_ref.py, tests/test_ln_ref_cpu.py and tests/test_ln_kernels_gpu.py")
L.append("(written by tools/text_rows_report.py from the files the tests append to when PSG_LN_REPORT names one)")
L.append("")
L.append("1. The constant of the y and dz bounds")
L.append("   Smallest c at which torch's own fp32 F.layer_norm on the CPU (autograd backward; bf16 operands pre-rounded, bf16 outputs")
L.append(f"   rounded) passes each bound against the fp64 reference: the largest over the {len(K.all_variants())} launches of tests/ln_cases.py.")
L.append("   x>y / x>dy    y         dz")
c = {(f[1], f[2]): float(f[3]) for f in rows if f[0] == "torch_c"}
for xd, od in K.PAIRS:
    p = f"{xd}>{od}"
    L.append(f"   {p:<13} {c[(p, 'y')]:<9.4g} {c[(p, 'dz')]:<9.4g}")
top = {f[1]: float(f[2]) for f in rows if f[0] == "torch_c_max"}
for n in ("y", "dz"):
    L.append(f"   C_TORCH {n} = {R.C_TORCH if top[n] == max(top.values()) else top[n]:.4g} (measured {top[n]:.4g})")
L.append(f"   C_TORCH = {R.C_TORCH:g}, C_LN = 4 x C_TORCH = {R.C_LN:g} (one value for both outputs)")
L.append("   The constant is fixed in tests/ln_ref.py so that every host holds the kernels to one bound; the CPU test requires this")
L.append("   measurement to lie within [0.8, 1] x C_TORCH on the host it runs on.  The largest value comes from N = 8, where a row")
L.append("   is one chunk.  (0: the error fits the output's own rounding and dz's c_acc reduction terms alone.  Those terms,")
L.append("   rstd (e1 + xa e2), stand outside C_LN and dominate the fp32 dz bound, as in the GroupNorm report: on the `offset` rows")
L.append("   they admit any rstd, so the one-pass variance is held by y alone.)")
L.append("")
L.append("2. torch's fp32 against the derived dgamma / dbeta bounds (row_ref.check, depth counted from the kernels): worst err / bound")
for f in rows:
    if f[0] == "torch_ratio":
        L.append(f"   {f[1]:<13} {f[2]:<7} {float(f[3]):.3g}")
L.append("")
L.append("3. Planted mistakes: the case each was asserted on and the outputs that left their bound")
mu = collections.OrderedDict()
for f in rows:
    if f[0] == "mutation":
        on = "rejected_on" in f
        mu.setdefault((f[1], " ".join(f[2:f.index("rejected_on")] if on else f[2:-1])), []).append(f[-1] if on else "")
for (m, case), outs in mu.items():
    L.append(f"   {m:<19} {case:<52} {' '.join(o for o in outs if o) or 'rejected'}")
L.append("")
L.append("4. Worst err / bound per kernel, dtypes and output, measured on an MI355X (0 = bit-exact comparison)")
over = []
for l in open(gpu):
    if l.startswith("gpu "):
        L.append("   " + l[4:].rstrip())
        f = l.split()
        if f[1] != "comparisons" and float(f[-1]) > 0.5:
            over.append(" ".join(f[1:-1]))
L.append(f"   Above 0.5 of the bound: {len(over)} entries" + (" - " + "; ".join(over) if over else "") + ".")
L.append("   Each of them is an output stored in bf16 (y in the launch's output type, dz in x's): round-to-nearest uses up to half an")
L.append("   ulp, 2^-8 relative just above a power of two, which is the whole of BF16_ROUND.  The bit identities are assertions of")
L.append("   the same run: second run, launch geometry (rows 37:41 of 150 against a 4-row launch), residual operand against")
L.append("   pre-added input, accumulate = prefill + result, NULL outputs, and psg_bert_embed_ln / psg_bert_embed_ln_bwd against")
L.append("   psg_layernorm / psg_layernorm_bwd on the fp32 rows formed by torch: all held, no discrepancy from FP contraction")
L.append("   between the instantiations.")
open(out, "w").write("\n".join(L) + "\n")
print("\n".join(L))
