"""Writes tests/golden/REPORT_conv_routes.txt from the figures the conv route tests append to the file PSG_CONV_REPORT names:
PSG_CONV_REPORT=cpu.txt pytest tests/test_conv_ref_cpu.py;  PSG_CONV_REPORT=gpu.txt pytest -m gpu tests/test_conv_routes_gpu.py;
python tools/conv_routes_report.py cpu.txt gpu.txt tests/golden/REPORT_conv_routes.txt

python tools/conv_routes_report.py --routes  rewrites tests/golden/conv_routes.json, the expected route of every case of
tests/conv_cases.py, from the library's psg_conv_route (host only) - for a deliberate planning change, to be read in the diff."""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import conv_cases as K
from tests import gemm_ref as R

if sys.argv[1:2] == ["--routes"]:
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.load()
    routes = {}
    for c in K.CASES:
        rc, rt = K.query_route(lib, c)
        assert rc == 0, (c["name"], rc, lib.psg_last_error())
        routes[c["name"]] = [list(l) for l in rt]
    with open(K.ROUTES_JSON, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in routes.items()) + "\n}\n")
    sys.exit(0)

cpu, gpu, out = sys.argv[1:4]
L = ["Conv forward / data-gradient route tests: the figures behind tests/conv_cases.py, tests/test_conv_ref_cpu.py and",
     "tests/test_conv_routes_gpu.py (written from the files the tests append to when PSG_CONV_REPORT names one)", ""]
L.append(f"1. The table: {len(K.CASES)} cases, {sum(len(K.expected_route(c['name'])) for c in K.CASES)} launches")
for l in open(cpu):
    if l.startswith(("sweep", "torch_f32", "act_approx")):
        L.append("   " + l.strip())
L.append("   torch's fp32 GEMM lies inside check()'s bound, which is therefore used unwidened for the fp32 launches")
L.append("")
L.append("2. Injected defects (CPU emulation at the table's shapes): defect -> cases whose comparison rejected it")
dd = collections.defaultdict(list)
for l in open(cpu):
    f = l.split()
    if f[0] == "defect":
        dd[f[1]].append(f[-1])
for k in sorted(dd):
    L.append(f"   {k:<24} {', '.join(dd[k])}")
L.append("   (a saved ReLU derivative is exactly 0 or 1, so its ratio is 0 where no element is wrong; the CPU test holds every ReLU case")
L.append("    to at least 10 % of its pre-activations on either side of zero and every tanh case to tanh' > 0.2 on 80 % of them)")
L.append("")
L.append("3. GPU: worst err / bound per route tuple (dtype, BM, BN, mode, split, tapcls, pw, epi_lds) and output, and the case that set it")
worst = {}
total, n = 0.0, 0
for l in open(gpu):
    r = json.loads(l)
    if "wall_s" in r:
        L.append(f"   whole file: {r['tests']} tests, {r['wall_s']:.1f} s from the first test to the last with the fp64 references (pytest reports about 2 s more: imports and collection) (slowest case {r['slowest']} {r['slowest_s']:.2f} s)")
        continue
    for key in r["keys"]:
        for name, v in r["ratios"].items():
            k = (tuple(key), name)
            if k not in worst or v > worst[k][0]:
                worst[k] = (v, r["case"])
for (key, name), (v, case) in sorted(worst.items(), key=lambda kv: (str(kv[0][0]), kv[0][1])):
    L.append(f"   {str(key):<44} {name:<7} {v:.4f}  {case}")
with open(out, "w") as f:
    f.write("\n".join(L) + "\n")
