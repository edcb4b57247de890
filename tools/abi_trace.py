"""Record every call a test run makes into libpsg_hip.so, in a form two source trees can be compared by.

    python tools/abi_trace.py --out TRACE tests/test_unet_gpu.py tests/test_vae_gpu.py ...     (from the tree's root)
    python tools/abi_trace.py --compare TRACE_A TRACE_B

After `_lib.load()` every function include/psg_hip.h declares (`_lib.ABI.functions`: the parsed parameter lists, which also say
which argument is the stream and which a workspace byte count) is replaced on the loaded library object by a recorder that
writes one line and then calls the function.  The given pytest node ids run in-process; at the start of every test the torch
seed and the dropout seed stream's counter are reset, so a test's calls do not depend on the tests before it.  A line holds
the entry name and, per argument: integers and floats in full (dropout seeds included); for a pointer whether it is null and
its address modulo 16 (alignment selects kernel routes); for a descriptor its fields, by the same rules; for the stream
whether it is the first stream seen or another; for a workspace byte count zero / non-zero (the pool only grows, so its size
depends on what ran before).  Two trees that load the same library (PSG_LIB_PATH) and give the same trace launch the same
kernels on the same operands.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.getcwd())


def _addr(v):
    if v is None:
        return 0
    if isinstance(v, int):
        return v
    if isinstance(v, C.c_void_p):
        return v.value or 0
    return C.addressof(v._obj) if hasattr(v, "_obj") else C.cast(v, C.c_void_p).value or 0      # byref(...) / other ctypes pointers


def _pointer(v):
    a = _addr(v)
    return "null" if a == 0 else f"p{a % 16}"


def _struct(p):
    out, d = [], (p.contents if hasattr(p, "contents") else p._obj)            # a POINTER instance or byref(desc)
    for name, typ in d._fields_:
        v = getattr(d, name)
        out.append(f"{name}=" + (_pointer(v) if typ is C.c_void_p else ("ws0" if v == 0 else "ws+") if name == "ws_bytes" else repr(v)))
    return "{" + " ".join(out) + "}"


class Recorder:
    def __init__(self, out):
        self.out, self.streams, self.calls = out, [], 0

    def wrap(self, name, fn, params):
        """params: the header's parameter list, [(ctypes type, C type text, name)] (_lib.ABI.functions)."""
        def call(*args):
            parts = []
            for a, (t, ctext, pname) in zip(args, params):
                if ctext == "psg_stream_t":
                    s = _addr(a)
                    if s not in self.streams:
                        self.streams.append(s)
                    parts.append("stream0" if self.streams[0] == s else "stream+")
                elif t is C.c_void_p:
                    parts.append(_pointer(a))
                elif hasattr(t, "contents"):
                    parts.append(_struct(a))
                elif ctext == "int64_t" and pname == "ws_bytes":
                    parts.append("ws0" if int(a) == 0 else "ws+")
                else:
                    parts.append(repr(float(a)) if t is C.c_float else repr(int(a)))
            self.out.write(name + " " + " ".join(parts) + "\n")
            self.calls += 1
            return fn(*args)
        return call

    # pytest plugin: one header line per test, seeds reset before its fixtures run
    def pytest_runtest_logstart(self, nodeid, location):
        import torch
        from pokemon_sprite_generator_amd import unet
        torch.manual_seed(0)
        unet._SeedStream.counter = 0
        self.out.write(f"## {nodeid}\n")


def compare(a, b):
    def load(path):
        tests, cur = {}, None
        for line in open(path):
            if line.startswith("## "):
                cur = tests.setdefault(line[3:].strip(), [])
            elif cur is not None:
                cur.append(line)
        return tests
    ta, tb = load(a), load(b)
    calls = bad = 0
    for t in sorted(set(ta) | set(tb)):
        la, lb = ta.get(t), tb.get(t)
        if la == lb:
            calls += len(la)
            continue
        bad += 1
        if la is None or lb is None:
            print(f"DIFF {t}: only in {'B' if la is None else 'A'}")
            continue
        i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        print(f"DIFF {t}: {len(la)} vs {len(lb)} calls, first difference at call {i}:\n  A: {la[i].strip() if i < len(la) else '-'}\n"
              f"  B: {lb[i].strip() if i < len(lb) else '-'}")
    print(f"{len(set(ta) | set(tb))} tests, {bad} differ, {calls} calls compared equal")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="TRACE")
    ap.add_argument("nodeids", nargs="*")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    import pytest
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.load()
    with open(args.out, "w") as out:
        rec = Recorder(out)
        for name, (_, params) in _lib.ABI.functions.items():
            setattr(lib, name, rec.wrap(name, getattr(lib, name), params))
        rc = pytest.main([*args.nodeids, "-q", "-m", "gpu", "-p", "no:cacheprovider"], plugins=[rec])
    print(f"{rec.calls} calls recorded, pytest exit code {int(rc)}")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
