"""Cases of psg_conv_wgrad_slim (csrc/conv_wgrad_slim.hip) shared by tests/test_conv_wgrad_slim_cpu.py and
tests/test_conv_wgrad_slim_gpu.py (test infrastructure; not a conftest).  A case is a dict of tests/wgrad_cases.py's kind, so
`wgrad_cases.make_desc` / `geom` build the psg_wgrad_desc that both entries take."""
from tests import wgrad_cases as W

TILE_H, TILE_W = 8, 16                                   # the kernel's output tile


def mk(name, **kw):
    c = dict(W.DEFAULTS)
    c.update(kw)
    c["name"] = name
    if c["W"] is None:
        c["W"] = c["H"]
    return c


def ntiles(c):
    return c["B"] * -(-c["H"] // TILE_H) * -(-c["W"] // TILE_W)


# Every Cout / Cin / kernel size of the contract's corners on a 5 x 7 grid, batch 3: M = 105 is no multiple of a K step (32) or
# of a tile (128) and every image border falls inside a tile; both row strides wider than the channels.
SMALL = [mk(f"s.k{ks}.i{cin}.o{cout}", B=3, H=5, W=7, Cin=cin, Cout=cout, ks=ks, ldx=8, lddy=16)
         for ks in (1, 3) for cin in (8, 32, 64, 128) for cout in (8, 32, 64)]
# 11 x 19: 2 x 2 tiles per image, so a halo comes from a neighbouring tile and a tile boundary lies inside the image
SMALL += [mk("s.k3.i40.o16.tiles", B=2, H=11, W=19, Cin=40, Cout=16, ks=3, ldx=0, lddy=8),
          mk("s.k1.i32.o32.tiles", B=2, H=11, W=19, Cin=32, Cout=32, ks=1, ldx=8, lddy=0)]
# (splits pin, accumulate, dbias, layout): each pin with accumulate and dbias on and off and both layouts
CONFIGS = [(s, acc, db, lay) for s in (1, 3) for acc, db, lay in ((False, True, "ohwi"), (True, False, "oihw"), (True, True, "oihw"), (False, False, "ohwi"))]
# M = 92 450 > 2^16: the plan's own slab count
LARGE = mk("l.k3.i32.o32.215", B=2, H=215, W=215, Cin=32, Cout=32, ks=3, dbias=True, layout="oihw")
