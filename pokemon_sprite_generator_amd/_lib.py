"""ctypes binding of libpsg_hip.so (the C ABI declared in include/psg_hip.h).

The product path has NO fallback: if the shared library is missing, any attempt
to run an op raises (``load()``), it never reroutes to a CPU or eager path.
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PSG_LIB_PATH") or os.path.join(_HERE, "libpsg_hip.so")   # override: A/B kernel builds in one GPU session
HEADER_PATH = os.path.join(_HERE, "..", "include", "psg_hip.h")


class PsgError(RuntimeError):
    pass


# ---------------------------------------------------------------------------
# The header is the one declaration of the ABI: prototypes, descriptor structs and constants are read from its text at
# import.  It is plain C (one prototype / field line / enum member per statement, /* */ comments), which the regular
# expressions below read exactly; anything they cannot place raises - nothing is skipped and no type is guessed.
# ---------------------------------------------------------------------------
BY_VALUE = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
            "psg_stream_t": C.c_void_p}
STRUCT_CLASS_NAMES = {"psg_conv_desc": "ConvDesc", "psg_wgrad_desc": "WgradDesc"}


class Abi:
    """functions: name -> (restype, [(ctypes type, C type text, parameter name)]); structs: C name -> ctypes.Structure
    class, whose _fields_ is the ordered [(field name, ctypes type)]; constants: enum members and integer #defines."""

    def __init__(self):
        self.functions, self.structs, self.constants = {}, {}, {}


def _oneline(decl):
    return " ".join(decl.split())


def _declarator(decl):
    """`const float *x` -> ("const float*", "x")"""
    m = re.fullmatch(r"(.*[\s*])(\w+)", _oneline(decl))
    ctext = re.sub(r"\s*\*\s*", "*", m.group(1)).strip() if m else ""
    if not re.fullmatch(r"(const )?\w+\**", ctext):
        raise PsgError(f"psg_hip.h: cannot split the declaration `{_oneline(decl)}`")
    return ctext, m.group(2)


def _ctype(ctext, structs, decl, is_return=False):
    const = ctext.startswith("const ")
    base = ctext[len("const "):] if const else ctext
    if base.endswith("*"):
        if is_return and ctext == "const char*":
            return C.c_char_p
        return C.POINTER(structs[base[:-1]]) if const and base[:-1] in structs else C.c_void_p
    if base not in BY_VALUE:
        raise PsgError(f"psg_hip.h: no ctypes mapping for the by-value type `{ctext}` in `{_oneline(decl)}`")
    return BY_VALUE[base]


def parse_header(text):
    abi = Abi()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PSG_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M):
        abi.constants[name] = int(value)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def enum(m):
        for member in filter(None, (s.strip() for s in m.group(1).split(","))):
            mm = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", member)
            if not mm:
                raise PsgError(f"psg_hip.h: enum member `{member}` is not written `NAME = <decimal integer>`")
            abi.constants[mm.group(1)] = int(mm.group(2))
        return ""
    text = re.sub(r"\benum\s+\w+\s*\{([^{}]*)\}\s*;", enum, text)

    def struct(m):
        fields = []
        for decl in filter(None, (s.strip() for s in m.group(1).split(";"))):       # `int32_t B, Hi, Wi, Cin`
            first, *more = decl.split(",")
            ctext, name = _declarator(first)
            if not all(re.fullmatch(r"\s*\w+\s*", n) for n in more):
                raise PsgError(f"psg_hip.h: cannot split the declaration `{_oneline(decl)}`")
            fields += [(n.strip(), _ctype(ctext, abi.structs, decl)) for n in [name] + more]
        abi.structs[m.group(2)] = type(STRUCT_CLASS_NAMES.get(m.group(2), m.group(2)), (C.Structure,),
                                       {"_fields_": fields, "__doc__": f"struct {m.group(2)} (include/psg_hip.h)."})
        return ""
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"\btypedef\s+[^;{}]*;", "", text)                     # plain typedefs (psg_stream_t): BY_VALUE names them
    text = re.sub(r'\bextern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    for decl in filter(None, (s.strip() for s in text.split(";"))):      # what is left must all be prototypes
        m = re.fullmatch(r"([^()]*)\(([^()]*)\)", decl)
        if not m:
            raise PsgError(f"psg_hip.h: cannot split the declaration `{_oneline(decl)}`")
        rtext, name = _declarator(m.group(1))
        params = [] if m.group(2).strip() == "void" else [_declarator(p) for p in m.group(2).split(",")]
        abi.functions[name] = (_ctype(rtext, abi.structs, decl, is_return=True),
                               [(_ctype(t, abi.structs, decl), t, n) for t, n in params])
    return abi


def read_header(path=HEADER_PATH):
    try:
        with open(path, encoding="utf-8") as f:
            text = f.read()
    except OSError as e:
        raise PsgError(f"cannot read the ABI header {path}: {e}") from None
    return parse_header(text)


ABI = read_header()
SIGNATURES = {name: (res, [p[0] for p in params]) for name, (res, params) in ABI.functions.items()}   # name -> (restype, argtypes)
ConvDesc, WgradDesc = ABI.structs["psg_conv_desc"], ABI.structs["psg_wgrad_desc"]


def _k(names):
    return [ABI.constants["PSG_" + n] for n in names.split()]


PSG_F32, PSG_BF16 = _k("F32 BF16")
OK, ERR_SHAPE, ERR_DTYPE, ERR_ALIGN, ERR_WORKSPACE, ERR_HIP, ERR_ARG = _k("OK ERR_SHAPE ERR_DTYPE ERR_ALIGN ERR_WORKSPACE ERR_HIP ERR_ARG")
ACT_NONE, ACT_SILU, ACT_GELU, ACT_RELU, ACT_TANH, ACT_QUICK_GELU = _k("ACT_NONE ACT_SILU ACT_GELU ACT_RELU ACT_TANH ACT_QUICK_GELU")
CONV_SAVE_DACT, CONV_DACT_MUL, CONV_GENERIC_EPILOGUE = _k("CONV_SAVE_DACT CONV_DACT_MUL CONV_GENERIC_EPILOGUE")
# enum psg_flag: bits of the per-step NaN/Inf flag word
FLAG_NOISY_BAD, FLAG_T_RANGE, FLAG_PRED_BAD, FLAG_LOSS_BAD, FLAG_FALLBACK, FLAG_INPUT_BAD, FLAG_SKIP_MASK = _k(
    "FLAG_NOISY_BAD FLAG_T_RANGE FLAG_PRED_BAD FLAG_LOSS_BAD FLAG_FALLBACK FLAG_INPUT_BAD FLAG_SKIP_MASK")

_lib = None
_inited = set()


def load():
    """dlopen libpsg_hip.so and declare every entry point.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PsgError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C pokemon_sprite_generator_amd/csrc`). There is no CPU/eager fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().psg_last_error()
        raise PsgError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def init(device_index: int):
    lib = load()
    if device_index not in _inited:
        check(lib.psg_init(int(device_index)), "psg_init")
        _inited.add(device_index)
    return lib


AVAIL_CUS = [256, 0]                     # mirror of (psg_set_available_cus, psg_set_reserve_rounds): ops caches split-K plans per value


def set_available_cus(device_index: int, n: int, rounds: int = 0):
    """psg_set_available_cus (+ psg_set_reserve_rounds) and the host-side mirror (n = 0: the whole chip)."""
    lib = init(device_index)
    check(lib.psg_set_available_cus(int(n)), "psg_set_available_cus")
    check(lib.psg_set_reserve_rounds(int(rounds)), "psg_set_reserve_rounds")
    AVAIL_CUS[0], AVAIL_CUS[1] = (256 if n == 0 else int(n)), int(rounds)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr():
    """The current HIP stream of the current device as a C pointer (honours `with torch.cuda.stream(...)`).  The raw
    accessor skips the Stream object `torch.cuda.current_stream()` builds: 8 us a call, ~1000 calls per train step."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(dt):
    if dt == torch.float32:
        return PSG_F32
    if dt == torch.bfloat16:
        return PSG_BF16
    raise PsgError(f"unsupported compute dtype {dt}")


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ---------------------------------------------------------------------------
# grow-only device workspace (one per (device, stream); all kernels on one stream run in order, so they share scratch)
# ---------------------------------------------------------------------------
class WorkspacePool:
    """key -> buffer, grown by replacement.  A captured hipGraph holds RAW POINTERS into the buffer of its capture stream, and
    torch recycles stream handles (a pool of 32 per device), so the rules are:
      * while frozen (a capture is open) a request that would replace a buffer raises - growth belongs to the eager warm-up;
      * a graph owner `hold()`s the buffer its capture used: it keeps a reference (the memory cannot be freed under the
        graph, whatever later happens to the key) and the key is marked held - a later, larger request on a recycled handle
        then allocates a NEW buffer for the key and leaves the held one alone instead of freeing it;
      * `drop()` (owner closed) releases the hold and, when the key's current buffer is the held one, the entry - so
        repeated graph runs do not leave one buffer per recycled stream behind."""

    def __init__(self, alloc):
        self._alloc = alloc
        self._bufs = {}
        self._held = {}          # key -> list of buffers graph owners still point into
        self.frozen = False

    def get(self, key, nbytes, *alloc_args):
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            if self.frozen:
                raise PsgError(f"workspace of {nbytes} bytes requested inside a graph capture but the warm-up sized "
                               f"{0 if buf is None else buf.numel()} on this stream: run the eager warm-up on the capture stream")
            buf = self._alloc(max(int(nbytes), 1 << 20), *alloc_args)
            self._bufs[key] = buf    # (a held predecessor stays alive through self._held and its owner)
        return buf

    def hold(self, key):
        buf = self._bufs.get(key)
        if buf is None:
            raise PsgError("hold_workspace: no workspace was sized on this stream (run the eager warm-up first)")
        self._held.setdefault(key, []).append(buf)
        return key, buf

    def drop(self, handle):
        key, buf = handle
        held = self._held.get(key, [])
        for i, b in enumerate(held):
            if b is buf:
                del held[i]
                break
        if not held:
            self._held.pop(key, None)
            if self._bufs.get(key) is buf:
                del self._bufs[key]

    def __len__(self):
        return len(self._bufs)


_pool = WorkspacePool(lambda n, device: torch.empty(n, dtype=torch.uint8, device=device))


def freeze_workspaces(on: bool):
    """While frozen (a hipGraph capture is open) a request that would REPLACE a workspace raises: kernels already captured
    keep pointing at the old buffer, so growth must have happened in the eager warm-up on the same stream."""
    _pool.frozen = bool(on)


def _ws_key(device):
    di = device.index if device.index is not None else torch.cuda.current_device()
    return (di, _raw_stream(di) if _raw_stream is not None else torch.cuda.current_stream(device).cuda_stream)


def workspace(nbytes: int, device):
    # one buffer per (device, stream): kernels on one stream run in order, so they can share scratch; a second
    # stream (ops: weight gradients overlapped with data gradients) gets its own
    return _pool.get(_ws_key(device), nbytes, device)


def hold_workspace(device):
    """For the owner of a captured graph, called on the capture stream after the capture: pins the buffer the captured launches
    point into (see WorkspacePool).  Returns a handle for `drop_workspace`."""
    return _pool.hold(_ws_key(device))


def drop_workspace(handle):
    if handle is not None:
        _pool.drop(handle)
