"""Border-class order (TapCls, csrc/conv_gemm_kernel.h) per layer: every stride-1 3x3 shape of the U-Net, forward (bias +
per-sample add, conv1's form) and data gradient, timed with the class form off (psg_conv_set_tapclass(0)) and forced on (2),
interleaved inside one process; the last column is what the tile plan (1, the default) chooses."""
import sys, time, torch
import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pokemon_sprite_generator_amd import ops, _lib
lib = _lib.init(0)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS, ROUNDS = 10, 3
shapes = [(27, 320, 320), (27, 640, 320), (14, 640, 640), (14, 1280, 640), (7, 1280, 1280), (7, 2560, 1280), (4, 1280, 1280), (4, 2560, 1280)]


def timeit(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


print("%-22s %-5s %9s %9s %7s %5s" % ("shape", "kind", "off us", "class us", "gain", "plan"))
tot = {0: 0.0, 2: 0.0, "plan": 0.0}
for H, Cin, Cout in shapes:
    x = torch.randn(B, H, H, Cin, device='cuda').bfloat16()
    w = torch.randn(Cout, Cin, 3, 3, device='cuda') * 0.02
    b = torch.randn(Cout, device='cuda')
    ra = torch.randn(B, Cout, device='cuda').bfloat16()
    xd = x.clone().requires_grad_(True)
    yd = ops.conv2d(xd, w, None)
    g = torch.randn_like(yd)
    kinds = {"fwd": lambda: ops.conv2d(x, w, b, rowadd=ra), "dgrad": lambda: torch.autograd.grad(yd, xd, g, retain_graph=True)}
    for kind, fn in kinds.items():
        t = {0: [], 2: []}
        with torch.no_grad() if kind == "fwd" else torch.enable_grad():
            for _ in range(ROUNDS):
                for mode in (0, 2):
                    _lib.check(lib.psg_conv_set_tapclass(mode), "tapclass")
                    t[mode].append(timeit(fn))
            _lib.check(lib.psg_conv_set_tapclass(1), "tapclass")
            c0 = lib.psg_conv_tapclass_launches()
            fn(); torch.cuda.synchronize()
            plan = lib.psg_conv_tapclass_launches() > c0
        a, c = min(t[0]), min(t[2])
        tot[0] += a; tot[2] += c; tot["plan"] += c if plan else a
        print("%-22s %-5s %9.1f %9.1f %6.1f%% %5s" % (f"{H}x{H} {Cin}->{Cout}", kind, a, c, 100.0 * (a - c) / a, "cls" if plan else "-"), flush=True)
print("sum (one launch each): off %.1f us, class %.1f us, plan %.1f us" % (tot[0], tot[2], tot["plan"]))
