"""torch.autograd.Function wrappers over the C ABI (libpsg_hip.so).

All activations are channels-last: a conv tensor is [B, H, W, C], a token tensor
[B, L, C]; the last dim is contiguous and rows have a uniform stride.  Every op
here launches hand-written HIP kernels on torch's current stream; PyTorch only
owns the memory.  There is no eager fallback: tensors must be on a GPU.
"""
import ctypes as C
import os
import struct
import threading

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_QUICK_GELU, ACT_RELU, ACT_SILU, ConvDesc, WgradDesc, check, dtype_code, ptr, stream_ptr

__all__ = ["conv2d", "conv4s2_relu", "reparam", "linear", "group_norm", "group_norm_split", "attention_self", "attention_cross", "attention_cross_longq",
           "cross_in_proj", "upsample_bilinear", "nchw_to_nhwc", "nchw_to_nhwc_grad", "nhwc_to_nchw", "image_out", "recon_loss", "max_pool2x2", "image_prep", "feature_l1", "kl_loss", "clip_prep", "attention_causal", "cosine_loss", "text_pool", "timestep_sinusoid", "WeightCache", "ACT_NONE", "ACT_SILU", "ACT_GELU", "ACT_RELU",
           "ACT_QUICK_GELU"]


def _lib_for(t):
    if not t.is_cuda:
        raise _lib.PsgError("pokemon_sprite_generator_amd ops need GPU tensors: the HIP kernels are the only implementation")
    return _lib.init(t.device.index if t.device.index is not None else torch.cuda.current_device())


class RowCopies:
    """Counter of the hidden `.contiguous()` copies `_rows` had to make (irregular strides / misaligned rows): each one is
    a full extra pass over an activation through HBM.  The U-Net path is expected to make none (asserted by
    tests/test_unet_gpu.py); PSG_WARN_COPIES=1 logs the shape and strides of every offender."""
    count = 0
    bytes = 0
    warn = os.environ.get("PSG_WARN_COPIES", "0") != "0"

    @classmethod
    def note(cls, t):
        cls.count += 1
        cls.bytes += t.numel() * t.element_size()
        if cls.warn:
            import warnings
            warnings.warn(f"psg ops: layout copy of a {tuple(t.shape)} tensor with strides {tuple(t.stride())} (ptr%16={t.data_ptr() % 16})")


def _rows(t):
    """Collapse [..., C] with uniform row stride to (rows, ld); copies (and counts it, RowCopies) if the layout is irregular."""
    if t.stride(-1) != 1:
        RowCopies.note(t)
        t = t.contiguous()
    C_ = t.shape[-1]
    ld = t.stride(-2) if t.dim() >= 2 else C_
    ok = True
    expect = ld
    for i in range(t.dim() - 2, -1, -1):
        if t.shape[i] != 1 and t.stride(i) != expect:
            ok = False
            break
        expect = expect * t.shape[i]
    if not ok or (t.data_ptr() % 16) != 0 or (ld % 8) != 0:
        RowCopies.note(t)
        t = t.contiguous()
        ld = C_
    return t, ld


# ---------------------------------------------------------------------------
# prepared-weight cache
# ---------------------------------------------------------------------------
W_OIHW, W_OHWI = _lib.ABI.constants["PSG_W_OIHW"], _lib.ABI.constants["PSG_W_OHWI"]


def weight_layout(t):
    """psg_w_layout of a weight / weight-gradient tensor's MEMORY order: OIHW (torch contiguous) or OHWI
    (torch channels_last, the kernels' native order — optim.ParamArena stores conv weights that way);
    None if it is neither (the caller makes a contiguous copy)."""
    if t.is_contiguous():
        return W_OIHW
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return W_OHWI
    return None


class ParamShadow:
    """Parameter -> (optim.ParamArena, index) for arenas that keep a bf16 shadow copy of the flat master buffer
    (written by the AdamW kernel in its own pass).  For an OHWI / 2-D weight whose K needs no padding the shadow
    slice IS the prepared forward weight, and the data-gradient operand is transposed from it (half the bytes)."""
    _map = {}

    @classmethod
    def register(cls, param, arena, index):
        cls._map[id(param)] = (arena, index, param)

    @classmethod
    def unregister(cls, arena):
        """Drop the entries that belong to `arena` (only those: another arena's parameters keep their shadow)."""
        for k in [k for k, e in cls._map.items() if e[0] is arena]:
            del cls._map[k]

    @classmethod
    def clear(cls):
        cls._map.clear()

    @classmethod
    def lookup(cls, param):
        e = cls._map.get(id(param))
        if e is None or e[2] is not param:
            return None
        arena, index, _ = e
        return arena.shadow_slice(index)        # bf16 1-D tensor in sync with the parameter, or None


class WeightCache:
    """fp32 master weight (OIHW or OHWI memory order) -> kernel-layout weights in the compute dtype.

    wf: [O][Kpad] with k=(kh,kw,ci) for the forward gather, wd: [I][Kpad'] with
    k=(kh,kw,co) for the data-gradient gather (psg_prep_weight).  Entries are
    keyed on the parameter's storage, its torch version counter and a global
    epoch that optimizers writing through raw pointers bump (invalidate()).
    """
    epoch = 0
    _entries = {}

    @classmethod
    def invalidate(cls):
        cls.epoch += 1

    @classmethod
    def clear(cls):
        cls._entries.clear()
        cls.epoch += 1

    @classmethod
    def drop(cls, params):
        """Release the prepared copies of these parameters only (their storage is about to move, or their module is gone)."""
        ids = {id(p) for p in params}
        ids |= {id(e[1]) for k, e in cls._entries.items() if isinstance(k, tuple) and k[0] in ids}      # what was `derived` from them
        for k in [k for k in cls._entries if k in ids or (isinstance(k, tuple) and k[0] in ids)]:
            del cls._entries[k]

    @classmethod
    def derived(cls, param, tag, build, fresh=False):
        """`build()`, an fp32 tensor made from `param` (a zero-padded copy) that goes through `conv2d` like any weight: rebuilt, and
        the predecessor's own entry dropped, when the parameter's stamp moves or on every call (`fresh`: a differentiable copy)."""
        key = (id(param), tag)
        stamp = (param.data_ptr(), param._version, cls.epoch, torch.float32, 0)
        ent = cls._entries.get(key)
        if ent is None or ent[0] != stamp or fresh:
            cls._entries.pop(id(ent[1]) if ent else None, None)
            ent = cls._entries[key] = (stamp, build(), None, param, None)
        return ent[1]

    @classmethod
    def get(cls, w, dtype, need_wd, pad_in=0):
        key = id(w)
        stamp = (w.data_ptr(), w._version, cls.epoch, dtype, pad_in)
        ent = cls._entries.get(key)
        if ent is not None and ent[0] == stamp and (ent[2] is not None or not need_wd):
            return ent[1], ent[2]
        lib = _lib_for(w)
        if ent is not None and ent[4] is not None and ent[0][0] == stamp[0] and ent[0][3] == dtype and ent[3] is w:
            # Same parameter, same storage, one optimizer step later, forward operand = the arena's bf16 shadow: everything
            # but the CONTENTS of wd is as it was - the shapes, the shadow view (AdamW rewrote it in place) and the wd buffer,
            # which is refilled in place.  (Rebuilding the entry cost ~25 us of host time per weight and step: 4 ms of a step
            # that is launch-bound below a per-GPU batch of ~64.)
            O, I, ks, code = ent[4]
            shadow = ParamShadow.lookup(w)
            if shadow is not None and shadow.data_ptr() == ent[1].data_ptr():
                wf, wd = ent[1], ent[2]
                if need_wd:
                    if wd is None:
                        wd = torch.empty((I, lib.psg_kpad(ks * ks * O, code)), dtype=dtype, device=w.device)
                    check(lib.psg_prep_weight(ptr(shadow), dtype_code(torch.bfloat16), W_OHWI, None, ptr(wd), O, I, ks, code, stream_ptr()),
                          "psg_prep_weight")
                else:
                    wd = None                      # (stale contents: dropped until a caller needs it again)
                cls._entries[key] = (stamp, wf, wd, w, ent[4])
                return wf, wd
        O, I = w.shape[0], w.shape[1] + pad_in
        ks = w.shape[2] if w.dim() == 4 else 1
        code = dtype_code(dtype)
        kpf = lib.psg_kpad(ks * ks * I, code)
        kpd = lib.psg_kpad(ks * ks * O, code)
        src = w.detach()
        if ks == 4:                                # psg_prep_weight takes 4x4 as OHWI, O and I multiples of 4 (pad_in: the image's 3 in 8)
            src = torch.nn.functional.pad(src.float(), (0, 0, 0, 0, 0, pad_in)).contiguous(memory_format=torch.channels_last)
        layout = weight_layout(src)
        shadow = None
        if dtype == torch.bfloat16 and kpf == ks * ks * I and O % 4 == 0 and I % 4 == 0 and (layout == W_OHWI or ks == 1) and not pad_in:
            shadow = ParamShadow.lookup(w)
        wd = torch.empty((I, kpd), dtype=dtype, device=w.device) if need_wd else None
        if shadow is not None:                     # the AdamW pass already wrote the forward operand
            wf = shadow.view(O, kpf)
            if need_wd:
                check(lib.psg_prep_weight(ptr(shadow), dtype_code(torch.bfloat16), W_OHWI, None, ptr(wd), O, I, ks, code, stream_ptr()),
                      "psg_prep_weight")
        else:
            wf = torch.empty((O, kpf), dtype=dtype, device=w.device)
            if layout is None:
                src, layout = src.contiguous(), W_OIHW
            check(lib.psg_prep_weight(ptr(src), dtype_code(torch.float32), layout, ptr(wf), ptr(wd), O, I, ks, code, stream_ptr()),
                  "psg_prep_weight")
        # (keep w alive so id() stays unique; the 5th field marks entries whose wf is the shadow: refreshable in place)
        cls._entries[key] = (stamp, wf, wd, w, (O, I, ks, code) if shadow is not None else None)
        return wf, wd


class GradSink:
    """Parameter -> persistent fp32 gradient view (optim.GradArena).  When a parameter is registered, the
    backward kernels write (first use in a step) or accumulate (later uses) its gradient straight into the
    view and autograd gets None: no per-step zero-fill and no AccumulateGrad read-modify-write pass over
    640 M values.  `on_ready(index)` is how the data-parallel reducer learns a gradient is final."""
    _map = {}

    class Entry:
        __slots__ = ("view", "written", "index", "on_ready", "param", "owner")

    @classmethod
    def register(cls, param, view, index, on_ready=None, owner=None):
        """Make `view` the gradient sink of `param`.  A parameter has ONE sink: registering it again from another
        owner (a second GradArena over the same model) displaces the first owner, which is told so
        (`owner.displaced(param)`) and refuses to step from then on instead of silently accumulating through
        autograd's AccumulateGrad into views nothing zeroes."""
        old = cls._map.get(id(param))
        if old is not None and old.param is param and old.owner is not None and old.owner is not owner:
            old.owner.displaced(param)
        e = cls.Entry()
        e.view, e.written, e.index, e.on_ready, e.param, e.owner = view, False, index, on_ready, param, owner
        cls._map[id(param)] = e
        return e

    @classmethod
    def unregister(cls, owner):
        """Remove the sinks registered by `owner` (and only those)."""
        for k in [k for k, e in cls._map.items() if e.owner is owner]:
            del cls._map[k]

    @classmethod
    def unregister_all(cls):
        cls._map.clear()

    @classmethod
    def begin_step(cls, owner=None):
        for e in cls._map.values():
            if owner is None or e.owner is owner:
                e.written = False

    @classmethod
    def get(cls, param):
        e = cls._map.get(id(param))
        return e if (e is not None and e.param is param) else None

    @classmethod
    def done(cls, e):
        e.written = True
        if e.on_ready is not None:
            e.on_ready(e.index)

    @classmethod
    def unwritten(cls, owner=None):
        return [e for e in cls._map.values() if not e.written and (owner is None or e.owner is owner)]


# The two descriptors are packed with struct.pack_into into per-thread buffers (backward runs on autograd's thread) and
# handed over as a pointer: one C call instead of ~30 ctypes field stores (8 us a launch, ~600 launches per train step).
_PACK_CODE = {C.c_int: "i", C.c_float: "f", C.c_int64: "q", C.c_uint64: "Q", C.c_void_p: "Q"}


def _desc_format(desc):
    return struct.Struct("<" + "".join(_PACK_CODE[t] for _, t in desc._fields_))


def _check_pack_order(desc, order):
    """The pack_into calls below are positional: `order` names what they pass, in their order, and must be the header's."""
    fields = tuple(n for n, _ in desc._fields_)
    if fields != tuple(order):
        raise _lib.PsgError(f"{desc.__name__}: the header declares the fields {fields} but ops.py packs {tuple(order)}")


_CONV_FMT, _WGRAD_FMT = _desc_format(ConvDesc), _desc_format(WgradDesc)
assert _CONV_FMT.size == C.sizeof(ConvDesc) and _WGRAD_FMT.size == C.sizeof(WgradDesc)
_tls = threading.local()


def _desc_bufs():
    b = getattr(_tls, "bufs", None)
    if b is None:
        cb, wb = C.create_string_buffer(_CONV_FMT.size), C.create_string_buffer(_WGRAD_FMT.size)
        b = _tls.bufs = (cb, C.cast(cb, C.POINTER(ConvDesc)), wb, C.cast(wb, C.POINTER(WgradDesc)))
    return b


_SPLITK = os.environ.get("PSG_CONV_SPLITK", "1") != "0"
_SPLITK_MAX_OUT = 1 << 23            # M x Cout above which a launch fills the chip anyway


class SplitKStats:
    """How many conv / linear launches were given a split-K workspace (tests, tools)."""
    launches = 0


# psg_conv_fwd_workspace_bytes validates the descriptor and evaluates the tile / split plan: per (geometry, dtype, CUs the
# planner counts on) that answer never changes, and on the launch-bound small-batch / sampler paths the second host call
# per launch was as long as the launch itself
_splitk_need = {}


_CONV_PACK_ORDER = ("dtype", "B", "Hi", "Wi", "Cin", "Ho", "Wo", "Cout", "ksize", "stride", "pad", "transposed", "act",
                    "alpha", "drop_p", "flags", "drop_seed",
                    "ldx", "ldy", "ld_rowadd", "ld_residual", "ld_preact", "ld_dact", "ldw",
                    "x", "w", "y", "bias", "rowadd", "residual", "preact", "dact_u", "ws", "ws_bytes")    # ws, ws_bytes: also the "<Qq" tail
_check_pack_order(ConvDesc, _CONV_PACK_ORDER)


def _conv_launch(lib, dtype, x, ldx, w, ldw, y, ldy, geom, Cin, Cout, transposed=False, bias=None, rowadd=None,
                 residual=None, ld_res=0, preact=None, dact_u=None, ld_dact=0, act=ACT_NONE, alpha=1.0, drop_p=0.0, seed=0, flags=0):
    B, Hi, Wi, Ho, Wo, ks, stride, pad = geom
    cb, cp, _, _ = _desc_bufs()
    # positional: edit _CONV_PACK_ORDER together with this argument list
    _CONV_FMT.pack_into(cb, 0, dtype_code(dtype), B, Hi, Wi, Cin, Ho, Wo, Cout, ks, stride, pad, int(transposed), act,
                        float(alpha), float(drop_p), int(flags), int(seed) & 0xFFFFFFFFFFFFFFFF,
                        ldx, ldy, rowadd.stride(0) if rowadd is not None else 0, ld_res if residual is not None else 0,
                        preact.stride(-2) if preact is not None else 0, ld_dact if dact_u is not None else 0, ldw,
                        x.data_ptr(), w if isinstance(w, int) else w.data_ptr(), y.data_ptr(),
                        bias.data_ptr() if bias is not None else 0, rowadd.data_ptr() if rowadd is not None else 0,
                        residual.data_ptr() if residual is not None else 0, preact.data_ptr() if preact is not None else 0,
                        dact_u.data_ptr() if dact_u is not None else 0, 0, 0)
    # small grids (sampling, small batches): offer a split-K workspace.  Only launches with few output elements are asked
    # about (one plan evaluation on the host).  A batch-256 train step asks for its 4x4 convs and its Linears up to 8 M
    # outputs, and the planner takes split-K for one of them, the ProjGroup's time-projection data gradient (M = 256)
    # (tests/test_gemm_b256_gpu.py records which).
    if B * Ho * Wo * Cout <= _SPLITK_MAX_OUT and _SPLITK:
        key = (dtype, geom, Cin, Cout, transposed, _lib.AVAIL_CUS[0], _lib.AVAIL_CUS[1])
        need = _splitk_need.get(key)
        if need is None:
            need = _splitk_need[key] = lib.psg_conv_fwd_workspace_bytes(cp)
        if need > 0:
            ws = _lib.workspace(need, x.device)
            struct.pack_into("<Qq", cb, _CONV_FMT.size - 16, ws.data_ptr(), ws.numel())
            SplitKStats.launches += 1
    check(lib.psg_conv_fwd(cp, stream_ptr()), "psg_conv_fwd")


_WGRAD_PACK_ORDER = ("dtype", "B", "Hi", "Wi", "Cin", "Ho", "Wo", "Cout", "ksize", "stride", "pad", "accumulate", "dw_layout",
                     "accumulate_bias", "scale", "reserved1", "ldx", "lddy", "x", "dy", "dw", "dbias", "ws", "ws_bytes")
_check_pack_order(WgradDesc, _WGRAD_PACK_ORDER)


_WGRAD_SLIM = os.environ.get("PSG_WGRAD_SLIM", "1") != "0"          # 0: every launch goes to psg_conv_wgrad (A/B)
_WGRAD_SLIM_MIN_SIDE, _WGRAD_SLIM_MIN_M = 64, 11664


class SlimStats:
    """How many weight-gradient launches went to psg_conv_wgrad_slim (tests, tools)."""
    launches = 0


def _wgrad_slim_route(dtype, geom, Cin, Cout):
    """Whether a weight-gradient launch goes to psg_conv_wgrad_slim (csrc/conv_wgrad_slim.hip) instead of psg_conv_wgrad:
    inside the slim entry's contract AND inside the set where it was measured faster - the one place that decides.

    Measured (tools/bench_wgrad_slim.py, MI355X, bf16, with dbias, interleaved A/B; DESIGN.md section 19, raw lines in
    profiles/wgrad_slim_bench.jsonl): the VAE decoder's blocks 4 and 5 and its image convolution - 108 x 108 and 215 x 215
    pixels, Cin in {32, 64, 128}, Cout in {8, 32, 64}, 3x3 and 1x1 - at batch 1, 2, 4 and 16 (M = 11 664 ... 739 600): on
    every one of the 36 shapes the slim kernel takes 0.22 - 0.69 of psg_conv_wgrad's time, more than that shape's
    round-to-round spread of either entry.  Adopted for exactly those channel counts on images of at least 64 x 64 pixels
    (the 8 x 16-pixel tiles of a smaller image are mostly border; nothing smaller was measured) from the smallest M measured
    up; everything else keeps psg_conv_wgrad, which is also the only fp32 path.

    No launch of the U-Net train step comes near: its convolutions run at 27 x 27 pixels and below (side < 64), and the two
    layers with a small channel count, the 8 -> 320 input and the 320 -> 8 output convolution, have Cout = 320 and Cin = 320;
    its Linears are 1 x 1 "images".  tests/test_gemm_b256_gpu.py and the step's launch count are unchanged."""
    B, Hi, Wi, Ho, Wo, ks, stride, pad = geom
    return (_WGRAD_SLIM and dtype == torch.bfloat16 and stride == 1 and ks in (1, 3) and Ho == Hi and Wo == Wi
            and Cout in (8, 32, 64) and Cin in (32, 64, 128)
            and Hi >= _WGRAD_SLIM_MIN_SIDE and Wi >= _WGRAD_SLIM_MIN_SIDE and B * Hi * Wi >= _WGRAD_SLIM_MIN_M)


def _wgrad_launch(lib, dtype, x, ldx, dy, lddy, dw, geom, Cin, Cout, accumulate=False, dbias=None, accumulate_bias=False, scale=1.0):
    """dw (+)= dy^T . gather(x); with `dbias` the same launch also produces the bias gradient (column sums of dy).  The
    descriptor is packed once for either entry: psg_conv_wgrad, or psg_conv_wgrad_slim where `_wgrad_slim_route` says so."""
    B, Hi, Wi, Ho, Wo, ks, stride, pad = geom
    layout = weight_layout(dw)
    out = dw
    if layout is None:                       # exotic strides: compute contiguous, copy back
        out, layout = torch.empty(dw.shape, dtype=dw.dtype, device=dw.device), W_OIHW
        if accumulate:
            out.copy_(dw)
    if dbias is not None and (dbias.dtype != torch.float32 or not dbias.is_contiguous() or dbias.numel() != Cout):
        raise _lib.PsgError("wgrad: dbias must be a contiguous fp32 [Cout] tensor")
    _, _, wb, wp = _desc_bufs()

    def pack(ws_ptr, ws_bytes):
        # positional: edit _WGRAD_PACK_ORDER together with this argument list
        _WGRAD_FMT.pack_into(wb, 0, dtype_code(dtype), B, Hi, Wi, Cin, Ho, Wo, Cout, ks, stride, pad, int(accumulate), layout,
                             int(accumulate_bias) if dbias is not None else 0, float(scale), 0, ldx, lddy,
                             x.data_ptr(), dy.data_ptr(), out.data_ptr(), dbias.data_ptr() if dbias is not None else 0, ws_ptr, ws_bytes)
    pack(0, 0)
    if _wgrad_slim_route(dtype, geom, Cin, Cout):
        query, entry, name = lib.psg_conv_wgrad_slim_workspace_bytes, lib.psg_conv_wgrad_slim, "psg_conv_wgrad_slim"
        SlimStats.launches += 1
    else:
        query, entry, name = lib.psg_conv_wgrad_workspace_bytes, lib.psg_conv_wgrad, "psg_conv_wgrad"
    need = query(wp)
    if need < 0:
        check(-1, name + "_workspace_bytes")
    if need > 0:
        ws = _lib.workspace(need, x.device)
        pack(ws.data_ptr(), ws.numel())
    check(entry(wp, stream_ptr()), name)
    if out is not dw:
        dw.copy_(out)


def _colsum(lib, a, lda, R, groups, cols, dtype, out_dtype, keep2d=False, out=None, accumulate=False):
    if out is None:
        out = torch.empty((groups, cols) if keep2d or groups > 1 else (cols,), dtype=out_dtype, device=a.device)
    need = lib.psg_colsum_workspace_bytes(R, groups, cols)
    ws = _lib.workspace(need, a.device)
    check(lib.psg_colsum(ptr(a), lda, ptr(out), cols, R, groups, cols, dtype_code(dtype), dtype_code(out_dtype), int(accumulate),
                         ptr(ws), ws.numel(), stream_ptr()), "psg_colsum")
    return out


class SideStream:
    """Second HIP stream for the weight-gradient GEMMs of backward: wgrad depends only on the saved input and dY and
    nothing else in backward depends on it, so it fills the tail waves of the data-gradient GEMM that runs next on
    the main stream (-1.5 % step time).  Used only for gradients that go to a GradSink (optim.GradArena): the arena's
    finalize() joins the stream before anything reads the gradients.  OFF by default since round 3 (PSG_WGRAD_STREAM=1
    enables it): it paid -1.5 % in round 1, when the data-gradient kernels left tail waves idle; with the round-3
    weight-gradient tiles two co-running GEMMs only take each other's CUs (same box, batch 256: 82.4 ms with the
    stream, 81.5 without)."""
    enabled = os.environ.get("PSG_WGRAD_STREAM", "0") != "0"
    _streams = {}
    used = False
    # Operands of the launches still in flight on the side stream.  Holding the Python reference does two things:
    # the buffer cannot be recycled, and - the part that matters - autograd's gradient accumulation never adds IN PLACE
    # into a tensor that something else still references (InputBuffer only re-uses a buffer whose use_count is 1).
    # Without it `d_res = dy` (returned by _ConvFn.backward while the side-stream wgrad still reads dy) could be
    # overwritten on the main stream by `dy += other_branch_gradient` under the wgrad's feet.
    _pending = []

    @classmethod
    def get(cls, device):
        k = device.index if device.index is not None else torch.cuda.current_device()
        s = cls._streams.get(k)
        if s is None:
            s = cls._streams[k] = torch.cuda.Stream(device=device)
        return s

    @classmethod
    def hold(cls, *tensors):
        cls._pending.extend(t for t in tensors if t is not None)
        cls.used = True

    @classmethod
    def join(cls, device):
        if cls.used:
            torch.cuda.current_stream(device).wait_stream(cls.get(device))
            cls.used = False
        cls._pending.clear()


def _param_out(param):
    """(out, accumulate, sink entry or None) for a parameter gradient: the registered sink view or a fresh tensor."""
    e = GradSink.get(param)
    if e is not None:
        return e.view, e.written, e
    return torch.empty_like(param), False, None


def _param_ret(out, e):
    """What autograd gets back for a gradient produced into `_param_out`'s tensor."""
    if e is not None:
        GradSink.done(e)
        return None
    return out


def _linear_geom(M):
    """The conv geometry (B, Hi, Wi, Ho, Wo, ks, stride, pad) of a Linear over M rows."""
    return (M, 1, 1, 1, 1, 1, 1, 0)


def _conv_geom(x, ks, stride, pad):
    """The conv geometry of x [B,Hi,Wi,Cin] under a ks x ks kernel: Ho / Wo are nn.Conv2d's (floor)."""
    B, Hi, Wi = x.shape[0], x.shape[1], x.shape[2]
    return (B, Hi, Wi, (Hi + 2 * pad - ks) // stride + 1, (Wi + 2 * pad - ks) // stride + 1, ks, stride, pad)


def _deliver_gemm_grads(lib, dtype, parts, weight, bias, want_w, want_b, scale=1.0, side_stream=False, keep=()):
    """The weight gradient and the (fused) bias gradient of a GEMM node, delivered: returns what autograd gets for
    (weight, bias) - None for a gradient that went to the parameter's GradSink view, else the tensor.

    `parts`: one (x, ldx, g, ldg, geom, Cin, Cout) per launch; several parts write consecutive row ranges of ONE packed
    parameter (the in-projection), which is marked done once, after the last launch.  `want_b` without `want_w` (frozen
    weight) takes the column sums of g instead (`scale` applied afterwards: rare).

    `side_stream`: the launches may hop to SideStream when it is enabled and the weight has a sink; `keep` are tensors to
    hold besides each part's g and x until the stream is joined (see SideStream._pending: _ConvFn returns dy itself as
    d_res).  Only _ConvFn and _FFNFn pass it.  What is known of why: when the second stream was added, _ConvFn got the hop
    and _CrossInProjFn, which already existed, did not; _FFNFn, added afterwards, copied conv's; _QKVFn, added last, did
    not.  No measurement of the hop exists for the two packed-projection nodes.  The stream is off by default and measured
    slower, so the split is kept as it is, not extended."""
    if not (want_w or want_b):
        return None, None
    bo, bacc, be = _param_out(bias) if want_b else (None, False, None)
    whole = len(parts) == 1
    dw = None
    if want_w:
        wo, wacc, we = _param_out(weight)
        side = SideStream.get(wo.device) if (side_stream and SideStream.enabled and we is not None) else None
        row = 0
        for x, ldx, g, ldg, geom, Cin, Cout in parts:
            dwp, dbp = (wo, bo) if whole else (wo[row:row + Cout], None if bo is None else bo[row:row + Cout])
            if side is not None:
                side.wait_stream(torch.cuda.current_stream(wo.device))
                with torch.cuda.stream(side):
                    _wgrad_launch(lib, dtype, x, ldx, g, ldg, dwp, geom, Cin, Cout, accumulate=wacc, dbias=dbp, accumulate_bias=bacc, scale=scale)
                g.record_stream(side); x.record_stream(side)
                SideStream.hold(g, x, *keep)
            else:
                _wgrad_launch(lib, dtype, x, ldx, g, ldg, dwp, geom, Cin, Cout, accumulate=wacc, dbias=dbp, accumulate_bias=bacc, scale=scale)
            row += Cout
        dw = _param_ret(wo, we)
    else:
        row = 0
        for x, ldx, g, ldg, geom, Cin, Cout in parts:
            out = bo if whole else bo[row:row + Cout]
            M = geom[0] * geom[3] * geom[4]
            if scale == 1.0:
                _colsum(lib, g, ldg, M, 1, Cout, dtype, torch.float32, out=out, accumulate=bacc)
            else:                      # (rare: frozen weight, trainable bias, gated output)
                t = _colsum(lib, g, ldg, M, 1, Cout, dtype, torch.float32).mul_(scale)
                out.add_(t) if bacc else out.copy_(t)
            row += Cout
    return dw, (_param_ret(bo, be) if want_b else None)


class _AffineGrads:
    """The (gamma, beta) gradients of a normalisation backward, delivered.  The constructor hands out where the kernel writes:
    `dgamma`, `dbeta` (None for an unwanted one) and the ONE `accumulate` flag the kernels take; after the launch `finish()`
    returns what autograd gets for (gamma, beta), as `_deliver_gemm_grads`, and reports the sink entries ready.  When the two
    entries disagree on `written`, `dbeta` is a zeroed temporary that `finish()` joins into beta's view."""

    def __init__(self, gamma, beta, want_g, want_b):
        self.go, gacc, self.ge = _param_out(gamma) if want_g else (None, False, None)
        self.bo, self.bacc, self.be = _param_out(beta) if want_b else (None, False, None)
        self.dgamma, self.accumulate = self.go, (gacc if want_g else self.bacc)
        self.dbeta = torch.zeros_like(self.bo) if (want_g and want_b and gacc != self.bacc) else self.bo

    def finish(self):
        if self.dbeta is not self.bo:
            self.bo.add_(self.dbeta) if self.bacc else self.bo.copy_(self.dbeta)
        return (_param_ret(self.go, self.ge) if self.go is not None else None), (_param_ret(self.bo, self.be) if self.bo is not None else None)


# ---------------------------------------------------------------------------
# producing into a slice of a larger buffer (the decoder's concat) and the skip tensors' gradient fan-in
# ---------------------------------------------------------------------------
class SeedSource:
    """The device word every dropout-drawing launch adds to its seed (psg_set_seed_source).  Seeds are launch arguments: a
    train step captured into a hipGraph would replay the same masks forever; with the source enabled the per-site seeds stay
    fixed from step to step (unet._SeedStream restarts its counter each step) and this word, advanced ON THE DEVICE at the end
    of every step, is what changes - eager steps and graph replays then draw identical masks."""
    _t = None
    _users = 0                              # acquire / release count (one per captured train-step graph)
    _STEP = -7046029254386353131            # 0x9E3779B97F4A7C15 as int64 (wraps)

    @classmethod
    def enabled(cls):
        return cls._t is not None

    @classmethod
    def enable(cls, device):
        if cls._t is None:
            lib = _lib.init(device.index if device.index is not None else torch.cuda.current_device())
            cls._t = torch.zeros(1, dtype=torch.int64, device=device)
            check(lib.psg_set_seed_source(ptr(cls._t)), "psg_set_seed_source")
        return cls._t

    @classmethod
    def acquire(cls, device):
        """One count per captured graph: the device word is baked into the captured launches' arguments and must stay alive
        (and keep advancing) until the LAST graph that reads it is closed."""
        cls._users += 1
        return cls.enable(device)

    @classmethod
    def release(cls):
        if cls._users > 0:
            cls._users -= 1
            if cls._users == 0:
                cls.disable()

    @classmethod
    def disable(cls):
        if cls._t is not None:
            check(_lib.load().psg_set_seed_source(None), "psg_set_seed_source")
            cls._t = None
        cls._users = 0

    @classmethod
    def advance(cls):
        if cls._t is not None:
            cls._t.add_(cls._STEP)


class OutSlot:
    """Where an op should produce its result: a row-strided view (same shape as the result) of a larger buffer.  A plain
    Python object on purpose - handed to an autograd Function as a tensor it would count as an INPUT returned as an output."""

    def __init__(self, view):
        self.view = view


def _out_rows(out, shape, dtype, device):
    """(tensor to write, its row stride): a fresh contiguous tensor, or the OutSlot's view after checking that it can be
    addressed as rows (uniform row stride, 16-byte aligned rows)."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device), shape[-1]
    v = out.view
    if tuple(v.shape) != tuple(shape) or v.dtype != dtype or v.device != device:
        raise _lib.PsgError(f"out slot {tuple(v.shape)} {v.dtype} does not match the result {tuple(shape)} {dtype}")
    ld = v.stride(-2)
    esz = v.element_size()
    ok = v.stride(-1) == 1 and (v.data_ptr() % 16) == 0 and (ld * esz) % 16 == 0
    expect = ld
    for i in range(v.dim() - 2, -1, -1):
        if v.shape[i] != 1 and v.stride(i) != expect:
            ok = False
        expect *= v.shape[i]
    if not ok:
        raise _lib.PsgError(f"out slot with strides {tuple(v.stride())} is not row-addressable")
    return v, ld


def sum_rows(a, b=None, c=None, out=None):
    """a (+ b (+ c)) over row-strided [..., C] tensors in one pass (psg_sum_rows); `out` may be a strided view."""
    lib = _lib_for(a)
    ar, lda = _rows(a)
    C_ = ar.shape[-1]
    rows = 1
    for n_ in ar.shape[:-1]:
        rows *= int(n_)
    br, ldb = _rows(b) if b is not None else (None, 0)
    cr, ldc = _rows(c) if c is not None else (None, 0)
    if out is None:
        out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    o, ldo = _out_rows(OutSlot(out), tuple(a.shape), a.dtype, a.device)
    check(lib.psg_sum_rows(ptr(ar), lda, ptr(br) if br is not None else None, ldb, ptr(cr) if cr is not None else None, ldc,
                           ptr(o), ldo, rows, C_, dtype_code(a.dtype), stream_ptr()), "psg_sum_rows")
    return out


class _ConcatSlotFn(torch.autograd.Function):
    """torch.cat([x, skip], dim=-1) where x ALREADY lies in buf[..., :C1] (its producer wrote it there through an OutSlot)
    and skip was copied into buf[..., C1:] when the buffer was made: forward hands out the buffer, backward the two
    slices of its gradient (views: the consumers take row-strided gradients)."""

    @staticmethod
    def forward(ctx, x, skip, holder):
        buf = holder.view
        C1 = x.shape[-1]
        if x.data_ptr() != buf.data_ptr() or x.stride() != buf[..., :C1].stride() or tuple(x.shape[:-1]) != tuple(buf.shape[:-1]):
            raise _lib.PsgError("concat_slot: x was not produced in the buffer's slot")
        ctx.C1 = C1
        return buf

    @staticmethod
    def backward(ctx, dcat):
        return dcat[..., :ctx.C1], dcat[..., ctx.C1:], None


class ConcatSlot:
    """The decoder's concat without the concat: `slot = ConcatSlot(skip, C1)` allocates [.., C1 + C2] and copies the skip
    half (one strided pass, psg_sum_rows); the op producing x gets `out=slot.out`; `slot.cat(x, skip)` is the node whose
    result is the full buffer (reference unet.py:480-504)."""

    def __init__(self, skip, C1):
        shape = tuple(skip.shape[:-1]) + (C1 + skip.shape[-1],)
        self.buf = torch.empty(shape, dtype=skip.dtype, device=skip.device)
        with torch.no_grad():
            sum_rows(skip.detach(), out=self.buf[..., C1:])
        self.out = OutSlot(self.buf[..., :C1])

    def cat(self, x, skip):
        return _ConcatSlotFn.apply(x, skip, OutSlot(self.buf))


class _Fan3Fn(torch.autograd.Function):
    """One tensor, three consumers: the three gradients are summed in ONE pass (fp32 sum, one rounding) instead of
    autograd's clone of the first (a strided concat-gradient slice) plus two adds."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, g0, g1, g2):
        gs = [g for g in (g0, g1, g2) if g is not None]
        if not gs:
            return None
        if len(gs) == 1:
            return gs[0]
        return sum_rows(gs[0], gs[1], gs[2] if len(gs) > 2 else None)


def fan3(x):
    """(x, x, x) for a skip tensor's three consumers (next encoder stage, two decoder blocks); see _Fan3Fn."""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return x, x, x
    return _Fan3Fn.apply(x)


# ---------------------------------------------------------------------------
# conv / linear
# ---------------------------------------------------------------------------
class _ConvFn(torch.autograd.Function):
    """y = residual + alpha * drop(act(conv(x, W) + bias + rowadd[b]))  — psg_conv_fwd / psg_conv_wgrad."""

    @staticmethod
    def forward(ctx, x, weight, bias, rowadd, residual, stride, act, alpha, drop_p, seed, out=None):
        lib = _lib_for(x)
        dtype = x.dtype
        is_conv = weight.dim() == 4
        Cout, Cin = weight.shape[0], weight.shape[1]
        ks = weight.shape[2] if is_conv else 1
        xr, ldx = _rows(x)
        if is_conv:
            geom = _conv_geom(x, ks, stride, 1 if ks == 3 else 0)
            out_shape = (geom[0], geom[3], geom[4], Cout)
        else:
            geom = _linear_geom(xr.numel() // xr.shape[-1])
            out_shape = tuple(x.shape[:-1]) + (Cout,)
        need_dx = ctx.needs_input_grad[0]
        wf, wd = WeightCache.get(weight, dtype, need_dx)
        y, ldy = _out_rows(out, out_shape, dtype, x.device)
        has_epi = (act != ACT_NONE)
        any_grad = any(ctx.needs_input_grad)
        preact = torch.empty(out_shape, dtype=dtype, device=x.device) if (has_epi and any_grad) else None
        res_r, ld_res = (None, 0)
        if residual is not None:
            res_r, ld_res = _rows(residual)
        ra = None
        if rowadd is not None:
            ra = rowadd if (rowadd.stride(-1) == 1 and rowadd.stride(0) % 4 == 0 and rowadd.data_ptr() % 16 == 0) else rowadd.contiguous()
        _conv_launch(lib, dtype, xr, ldx, wf, 0, y, ldy, geom, Cin, Cout, bias=bias, rowadd=ra, residual=res_r, ld_res=ld_res,
                     preact=preact, act=act, alpha=alpha, drop_p=drop_p, seed=seed)
        ctx.save_for_backward(xr, weight, preact)
        ctx.bias_param, ctx.weight_param = bias, weight
        ctx.meta = (geom, Cin, Cout, ldx, act, alpha, drop_p, seed, bias is not None, rowadd is not None, residual is not None, tuple(x.shape), wd)
        return y

    @staticmethod
    def backward(ctx, dy):
        xr, weight, preact = ctx.saved_tensors
        geom, Cin, Cout, ldx, act, alpha, drop_p, seed, has_bias, has_ra, has_res, x_shape, wd = ctx.meta
        B, Hi, Wi, Ho, Wo, ks, stride, pad = geom
        lib = _lib_for(dy)
        dtype = dy.dtype
        dyr, lddy = _rows(dy)
        M = B * Ho * Wo
        d_res = dy if has_res else None
        # gradient w.r.t. the pre-epilogue accumulator; a pure output gate (alpha only) is folded into the dgrad
        # epilogue and the wgrad scale instead of a pass over dy
        gate = 1.0
        if act == ACT_NONE and drop_p == 0.0 and alpha != 1.0 and not has_ra:
            gate = float(alpha)
            g, ldg = dyr, lddy
        elif act != ACT_NONE or drop_p > 0.0 or alpha != 1.0:
            g = torch.empty((M, Cout), dtype=dtype, device=dy.device)
            check(lib.psg_epilogue_bwd(ptr(dyr), lddy, ptr(preact), Cout, ptr(g), Cout, M, Cout, act, float(alpha), float(drop_p),
                                       int(seed), dtype_code(dtype), stream_ptr()), "psg_epilogue_bwd")
            ldg = Cout
        else:
            g, ldg = dyr, lddy
        dx = dw = db = dra = None
        if ctx.needs_input_grad[0]:
            if wd is None:
                _, wd = WeightCache.get(weight, dtype, True)
            dx = torch.empty(x_shape, dtype=dtype, device=dy.device)
            tgeom = (B, Ho, Wo, Hi, Wi, ks, stride, pad)     # gather source = dY grid, result = input grid
            _conv_launch(lib, dtype, g, ldg, wd, 0, dx, Cin, tgeom, Cout, Cin, transposed=True, alpha=gate)
        # one launch: weight gradient + (fused) bias gradient, straight into the gradient arena when registered
        dw, db = _deliver_gemm_grads(lib, dtype, [(xr, ldx, g, ldg, geom, Cin, Cout)], ctx.weight_param, ctx.bias_param,
                                   ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2], scale=gate, side_stream=True, keep=(dy,))
        if has_ra and ctx.needs_input_grad[3]:
            dra = _colsum(lib, g, ldg, Ho * Wo, B, Cout, dtype, dtype, keep2d=True)
        return dx, dw, db, dra, d_res, None, None, None, None, None, None


class _NoNode:
    """An autograd ctx's stand-in while grad mode is off: `_node` runs the node's forward body as it is, without the cost of
    `Function.apply` per launch (a batch-1 VAE forward is host-bound); nothing is kept for a backward."""

    def __init__(self, args):
        self.needs_input_grad = [getattr(a, "requires_grad", False) for a in args]      # as apply would say

    def save_for_backward(self, *tensors):
        pass


def _node(fn, *args):
    return fn.apply(*args) if torch.is_grad_enabled() else fn.forward(_NoNode(args), *args)


def conv2d(x, weight, bias=None, stride=1, rowadd=None, residual=None, act=ACT_NONE, alpha=1.0, drop_p=0.0, seed=0, out=None):
    """x: [B,H,W,Cin] channels-last; weight: fp32 OIHW parameter (3x3 pad 1, or 1x1).  nn.Conv2d of unet.py.
    `out`: a row-strided tensor of the output's shape to produce the result in (`OutSlot`, see `concat_slot`)."""
    return _node(_ConvFn, x, weight, bias, rowadd, residual, stride, act, alpha, drop_p, seed, out)


def linear(x, weight, bias=None, residual=None, act=ACT_NONE, alpha=1.0, drop_p=0.0, seed=0, out=None):
    """x: [..., Cin]; weight: fp32 [Cout, Cin] parameter.  nn.Linear of unet.py, with the fused epilogue."""
    return _node(_ConvFn, x, weight, bias, None, residual, 1, act, alpha, drop_p, seed, out)


class _Conv4s2Fn(torch.autograd.Function):
    """y = relu(conv(x, W, kernel 4, stride 2, pad 1 | 2) + bias) - the VAE encoder's downsampling convolutions
    (vae_decoder.py:78-89).  Forward: psg_conv_fwd, the frozen encoder's launch.  Backward: psg_epilogue_bwd on the SAVED
    OUTPUT ([y > 0] is [u > 0] for ReLU: no pre-activation is kept), psg_conv4s2_dgrad (skipped when x needs no gradient: the
    image conv) and psg_conv4s2_wgrad (weight + bias gradient in one pass, delivered like `_deliver_gemm_grads`).  x may
    carry more channels than the weight (the image's 3 in 8 columns): the extra ones are zero and get no weight gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, pad):
        lib = _lib_for(x)
        dtype = x.dtype
        Cout, cin_real = weight.shape[0], weight.shape[1]
        Cin = x.shape[-1]
        if weight.dim() != 4 or weight.shape[2] != 4 or weight.shape[3] != 4 or Cin < cin_real:
            raise _lib.PsgError(f"conv4s2_relu: weight {tuple(weight.shape)} on an input of {Cin} channels")
        xr, ldx = _rows(x)
        geom = _conv_geom(x, 4, 2, pad)
        wf, wd = WeightCache.get(weight, dtype, ctx.needs_input_grad[0], pad_in=Cin - cin_real)
        y = torch.empty((geom[0], geom[3], geom[4], Cout), dtype=dtype, device=x.device)
        _conv_launch(lib, dtype, xr, ldx, wf, 0, y, Cout, geom, Cin, Cout, bias=bias, act=ACT_RELU)
        ctx.save_for_backward(xr, y)
        ctx.weight_param, ctx.bias_param = weight, bias
        ctx.meta = (geom, Cin, cin_real, Cout, ldx, tuple(x.shape), wd)
        return y

    @staticmethod
    def backward(ctx, dy):
        xr, y = ctx.saved_tensors
        geom, Cin, cin_real, Cout, ldx, x_shape, wd = ctx.meta
        B, Hi, Wi, Ho, Wo, _, _, pad = geom
        weight, bias = ctx.weight_param, ctx.bias_param
        lib = _lib_for(dy)
        dtype = dy.dtype
        code = dtype_code(dtype)
        dyr, lddy = _rows(dy)
        M = B * Ho * Wo
        g = torch.empty((M, Cout), dtype=dtype, device=dy.device)
        check(lib.psg_epilogue_bwd(ptr(dyr), lddy, ptr(y), Cout, ptr(g), Cout, M, Cout, ACT_RELU, 1.0, 0.0, 0, code, stream_ptr()),
              "psg_epilogue_bwd")
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x_shape, dtype=dtype, device=dy.device)
            check(lib.psg_conv4s2_dgrad(ptr(g), Cout, ptr(wd), ptr(dx), Cin, B, Hi, Wi, Cin, Ho, Wo, Cout, pad, code, stream_ptr()),
                  "psg_conv4s2_dgrad")
        want_w, want_b = ctx.needs_input_grad[1], bias is not None and ctx.needs_input_grad[2]
        bo, bacc, be = _param_out(bias) if want_b else (None, False, None)
        if want_w:
            wo, wacc, we = _param_out(weight)
            layout, out = weight_layout(wo), wo
            if layout is None:                       # exotic strides: compute contiguous, copy back
                out, layout = torch.empty(wo.shape, dtype=wo.dtype, device=wo.device), W_OIHW
                if wacc:
                    out.copy_(wo)
            need = lib.psg_conv4s2_wgrad_workspace_bytes(B, Ho, Wo, Cin, Cout, code)
            if need < 0:
                check(-1, "psg_conv4s2_wgrad_workspace_bytes")
            ws = _lib.workspace(need, dy.device)
            check(lib.psg_conv4s2_wgrad(ptr(xr), ldx, ptr(g), Cout, ptr(out), layout, cin_real, ptr(bo), B, Hi, Wi, Cin, Ho, Wo, Cout, pad,
                                        int(wacc), int(bacc), code, ptr(ws), ws.numel(), stream_ptr()), "psg_conv4s2_wgrad")
            if out is not wo:
                wo.copy_(out)
            dw = _param_ret(wo, we)
        elif want_b:                                 # (frozen weight, trainable bias)
            _colsum(lib, g, Cout, M, 1, Cout, dtype, torch.float32, out=bo, accumulate=bacc)
        if want_b:
            db = _param_ret(bo, be)
        return dx, dw, db, None


def conv4s2_relu(x, weight, bias, pad):
    """relu(nn.Conv2d(kernel_size=4, stride=2, padding=pad)(x)) on channels-last x [B,H,W,Cin >= weight's]; weight: the fp32
    OIHW parameter."""
    return _Conv4s2Fn.apply(x, weight, bias, pad)


class _ReparamFn(torch.autograd.Function):
    """latent = mu + eps * exp(0.5 logvar) in fp32 (psg_reparam_f32, vae_decoder.py:120-123); backward: psg_reparam_bwd_f32."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        lib = _lib_for(mu)
        if mu.shape != logvar.shape or mu.shape != eps.shape:
            raise _lib.PsgError(f"reparam: shapes {tuple(mu.shape)}, {tuple(logvar.shape)}, {tuple(eps.shape)} differ")
        m, lv, e = mu.detach().contiguous().float(), logvar.detach().contiguous().float(), eps.detach().contiguous().float()
        out = torch.empty_like(m)
        check(lib.psg_reparam_f32(ptr(m), ptr(lv), ptr(e), ptr(out), m.numel(), stream_ptr()), "psg_reparam_f32")
        ctx.save_for_backward(lv, e)
        return out

    @staticmethod
    def backward(ctx, dlat):
        lv, e = ctx.saved_tensors
        lib = _lib_for(dlat)
        d = dlat.contiguous().float()
        dmu = torch.empty_like(lv) if ctx.needs_input_grad[0] else None
        dlv = torch.empty_like(lv) if ctx.needs_input_grad[1] else None
        if dmu is not None or dlv is not None:
            check(lib.psg_reparam_bwd_f32(ptr(d), ptr(lv), ptr(e), ptr(dmu), ptr(dlv), 0, d.numel(), stream_ptr()), "psg_reparam_bwd_f32")
        return dmu, dlv, None


def reparam(mu, logvar, eps):
    """The VAE's reparameterised sample mu + eps * exp(0.5 logvar) (fp32), differentiable in mu and logvar."""
    return _ReparamFn.apply(mu, logvar, eps)


class _QKVFn(torch.autograd.Function):
    """qkv = x . [Wq; Wk; Wv]^T + [bq; bk; bv] as ONE GEMM over a packed prepared weight (BERT's self-attention input:
    query, key and value stay three parameters with three gradients).  `packed` = (wf [3H][Kpad], fp32 bias [3H],
    wd [Cin][Kpad'] for the data gradient), prepared by the caller from the three weights.  Backward: one data-gradient
    GEMM over wd, three weight-gradient launches reading the column slices of dqkv (bias gradients fused)."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, packed):
        lib = _lib_for(x)
        wf, bcat, wd = packed
        xr, ldx = _rows(x)
        Cin, H = wq.shape[1], wq.shape[0]
        M = xr.numel() // xr.shape[-1]
        y = torch.empty(tuple(x.shape[:-1]) + (3 * H,), dtype=x.dtype, device=x.device)
        geom = _linear_geom(M)
        _conv_launch(lib, x.dtype, xr, ldx, wf, 0, y, 3 * H, geom, Cin, 3 * H, bias=bcat)
        ctx.save_for_backward(xr, wd)
        ctx.params = (wq, bq, wk, bk, wv, bv)
        ctx.meta = (geom, Cin, H, ldx, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        xr, wd = ctx.saved_tensors
        geom, Cin, H, ldx, x_shape = ctx.meta
        lib = _lib_for(dy)
        dtype = dy.dtype
        g, ldg = _rows(dy)
        g2 = g.view(-1, g.shape[-1]) if ldg == g.shape[-1] else g
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x_shape, dtype=dtype, device=dy.device)
            _conv_launch(lib, dtype, g, ldg, wd, 0, dx, Cin, geom, 3 * H, Cin, transposed=True)
        grads = []
        for i in range(3):
            gi = g2[..., i * H:(i + 1) * H]                  # a column slice of dqkv: same row stride, start moved
            grads += _deliver_gemm_grads(lib, dtype, [(xr, ldx, gi, ldg, geom, Cin, H)], ctx.params[2 * i], ctx.params[2 * i + 1],
                                       ctx.needs_input_grad[1 + 2 * i], ctx.needs_input_grad[2 + 2 * i])
        return (dx, *grads, None)


def qkv_linear(x, wq, bq, wk, bk, wv, bv, packed):
    """x [..., Cin] -> packed [..., 3H] projections (query | key | value columns), see _QKVFn."""
    return _QKVFn.apply(x, wq, bq, wk, bk, wv, bv, packed)


def prep_qkv(wq, wk, wv, bq, bk, bv, dtype, need_wd):
    """The `packed` operand of qkv_linear: the three [H][Cin] fp32 weights as one prepared forward weight, the fp32 bias,
    and (need_wd) the prepared data-gradient weight."""
    lib = _lib_for(wq)
    src = torch.cat([wq.detach(), wk.detach(), wv.detach()], 0).float().contiguous()
    O, I = src.shape
    code = dtype_code(dtype)
    wf = torch.empty((O, lib.psg_kpad(I, code)), dtype=dtype, device=src.device)
    wd = torch.empty((I, lib.psg_kpad(O, code)), dtype=dtype, device=src.device) if need_wd else None
    check(lib.psg_prep_weight(ptr(src), dtype_code(torch.float32), W_OIHW, ptr(wf), ptr(wd), O, I, 1, code, stream_ptr()), "psg_prep_weight")
    return wf, torch.cat([bq.detach(), bk.detach(), bv.detach()]).float().contiguous(), wd


_FFN_SAVE_DACT = os.environ.get("PSG_FFN_SAVE_DACT", "1") != "0"     # 0: save u, re-evaluate gelu'(u) and the mask in backward (A/B)
_GN_SPLIT = os.environ.get("PSG_GN_SPLIT", "1") != "0"               # 0: plain GroupNorm node, autograd adds the bypass gradient (A/B)


class _FFNFn(torch.autograd.Function):
    """y = x + alpha * drop2(W2 . drop1(gelu(W1 x + b1)) + b2)   - the FFN of CrossAttentionBlock (unet.py:176-187, 250).

    One node instead of two `_ConvFn`s so that backward can use the kernels' fused forms: the data gradient of the
    second Linear is produced ALREADY multiplied by GELU'(u) and the first dropout mask (psg_conv_fwd's dact_u
    form: no pass over the [M, hidden] gradient), and the residual branch's gradient is added in the epilogue of the
    first Linear's data gradient (no autograd add)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, alpha, drop_p, seed1, seed2, out=None):
        lib = _lib_for(x)
        dtype = x.dtype
        C, Hd = w1.shape[1], w1.shape[0]
        xr, ldx = _rows(x)
        M = xr.numel() // C
        need = any(ctx.needs_input_grad)
        wf1, wd1 = WeightCache.get(w1, dtype, need)
        wf2, wd2 = WeightCache.get(w2, dtype, need)
        u = torch.empty((M, Hd), dtype=dtype, device=x.device) if need else None
        hmid = torch.empty((M, Hd), dtype=dtype, device=x.device)
        y, ldy = _out_rows(out, tuple(x.shape), dtype, x.device)
        g1 = _linear_geom(M)
        # `u` receives gelu'(W1 x + b1) * mask1 / (1 - p), not the pre-activation: backward multiplies by it
        _conv_launch(lib, dtype, xr, ldx, wf1, 0, hmid, Hd, g1, C, Hd, bias=b1, preact=u, act=ACT_GELU, drop_p=drop_p, seed=seed1,
                     flags=_lib.CONV_SAVE_DACT if (u is not None and _FFN_SAVE_DACT) else 0)
        _conv_launch(lib, dtype, hmid, Hd, wf2, 0, y, ldy, g1, Hd, C, bias=b2, residual=xr, ld_res=ldx, alpha=alpha, drop_p=drop_p, seed=seed2)
        ctx.save_for_backward(xr, u, hmid, w1, w2)
        ctx.params = (w1, b1, w2, b2)
        ctx.meta = (M, C, Hd, ldx, alpha, drop_p, seed1, seed2, tuple(x.shape), wd1, wd2)
        return y

    @staticmethod
    def backward(ctx, dy):
        xr, u, hmid, w1, w2 = ctx.saved_tensors
        w1p, b1p, w2p, b2p = ctx.params
        M, C, Hd, ldx, alpha, drop_p, seed1, seed2, x_shape, wd1, wd2 = ctx.meta
        lib = _lib_for(dy)
        dtype = dy.dtype
        dyr, lddy = _rows(dy)
        geo = _linear_geom(M)
        if wd1 is None:
            _, wd1 = WeightCache.get(w1, dtype, True)
        if wd2 is None:
            _, wd2 = WeightCache.get(w2, dtype, True)
        # gradient w.r.t. the second Linear's accumulator (dropout 2 and the 0.6 gate)
        g2 = torch.empty((M, C), dtype=dtype, device=dy.device)
        check(lib.psg_epilogue_bwd(ptr(dyr), lddy, None, C, ptr(g2), C, M, C, ACT_NONE, float(alpha), float(drop_p), int(seed2),
                                   dtype_code(dtype), stream_ptr()), "psg_epilogue_bwd")
        # d/du of the first Linear's pre-activation: dgrad of Linear 2 with the backward-form epilogue
        gu = torch.empty((M, Hd), dtype=dtype, device=dy.device)
        if _FFN_SAVE_DACT:
            _conv_launch(lib, dtype, g2, C, wd2, 0, gu, Hd, geo, C, Hd, transposed=True, dact_u=u, ld_dact=Hd, flags=_lib.CONV_DACT_MUL)
        else:
            _conv_launch(lib, dtype, g2, C, wd2, 0, gu, Hd, geo, C, Hd, transposed=True, dact_u=u, ld_dact=Hd, act=ACT_GELU, drop_p=drop_p, seed=seed1)

        # (a Linear whose weight OR bias trains gets both gradients from the one fused launch)
        dx = None
        need2, need1 = ctx.needs_input_grad[3] or ctx.needs_input_grad[4], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dw2, db2 = _deliver_gemm_grads(lib, dtype, [(hmid, Hd, g2, C, geo, Hd, C)], w2p, b2p, need2, need2, side_stream=True)
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x_shape, dtype=dtype, device=dy.device)
            # dx = W1^T gu + dy (the residual branch's gradient rides in the epilogue)
            _conv_launch(lib, dtype, gu, Hd, wd1, 0, dx, C, geo, Hd, C, transposed=True, residual=dyr, ld_res=lddy)
        dw1, db1 = _deliver_gemm_grads(lib, dtype, [(xr, ldx, gu, Hd, geo, C, Hd)], w1p, b1p, need1, need1, side_stream=True)
        return dx, dw1, db1, dw2, db2, None, None, None, None, None


def ffn(x, w1, b1, w2, b2, alpha, drop_p=0.0, seed1=0, seed2=0, out=None):
    """x + alpha * drop(W2 drop(gelu(W1 x + b1)) + b2), fused forward epilogues and backward forms (see _FFNFn)."""
    return _FFNFn.apply(x, w1, b1, w2, b2, alpha, drop_p, seed1, seed2, out)


class _CrossInProjFn(torch.autograd.Function):
    """Packed MHA in-projection for cross-attention (unet.py:235 -> F.multi_head_attention_forward):
    q = xn @ W[:E]^T + b[:E];  kv = tp @ W[E:]^T + b[E:]  with ONE packed parameter [3E, E]."""

    @staticmethod
    def forward(ctx, xn, tp, weight, bias):
        lib = _lib_for(xn)
        dtype = xn.dtype
        E = weight.shape[1]
        wf, wd = WeightCache.get(weight, dtype, ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        xr, ldx = _rows(xn)
        tr, ldt = _rows(tp)
        gq, gk = _linear_geom(xn.numel() // E), _linear_geom(tp.numel() // E)
        q = torch.empty(tuple(xn.shape[:-1]) + (E,), dtype=dtype, device=xn.device)
        kv = torch.empty(tuple(tp.shape[:-1]) + (2 * E,), dtype=dtype, device=xn.device)
        kp = wf.shape[1]
        esz = wf.element_size()
        _conv_launch(lib, dtype, xr, ldx, wf.data_ptr(), 0, q, E, gq, E, E, bias=bias[:E])
        _conv_launch(lib, dtype, tr, ldt, wf.data_ptr() + E * kp * esz, 0, kv, 2 * E, gk, E, 2 * E, bias=bias[E:])
        ctx.save_for_backward(xr, tr, weight)
        ctx.bias_param, ctx.weight_param = bias, weight
        ctx.meta = (E, ldx, ldt, gq, gk, tuple(xn.shape), tuple(tp.shape), wd, wf)
        return q, kv

    @staticmethod
    def backward(ctx, dq, dkv):
        xr, tr, weight = ctx.saved_tensors
        E, ldx, ldt, gq, gk, xs, ts, wd, wf = ctx.meta
        lib = _lib_for(dq)
        dtype = dq.dtype
        dqr, lddq = _rows(dq)
        dkr, lddk = _rows(dkv)
        if wd is None:
            _, wd = WeightCache.get(weight, dtype, True)
        kpd = wd.shape[1]
        esz = wd.element_size()
        dxn = dtp = None
        if ctx.needs_input_grad[0]:
            dxn = torch.empty(xs, dtype=dtype, device=dq.device)
            _conv_launch(lib, dtype, dqr, lddq, wd.data_ptr(), kpd, dxn, E, gq, E, E, transposed=True)
        if ctx.needs_input_grad[1]:
            dtp = torch.empty(ts, dtype=dtype, device=dq.device)
            _conv_launch(lib, dtype, dkr, lddk, wd.data_ptr() + E * esz, kpd, dtp, E, gk, 2 * E, E, transposed=True)
        # rows [:E] of the packed parameter from the queries, rows [E:] from the text tokens
        dw, db = _deliver_gemm_grads(lib, dtype, [(xr, ldx, dqr, lddq, gq, E, E), (tr, ldt, dkr, lddk, gk, E, 2 * E)],
                                   ctx.weight_param, ctx.bias_param, ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        return dxn, dtp, dw, db


def cross_in_proj(xn, tp, weight, bias):
    return _CrossInProjFn.apply(xn, tp, weight, bias)


# ---------------------------------------------------------------------------
# the 17 ResBlocks' time_proj / text_proj as TWO GEMMs (unet.py:83-86,119-124)
# ---------------------------------------------------------------------------
class _SplitColsFn(torch.autograd.Function):
    """[B, sum C] -> 17 column slices (views); backward = ONE concatenation of the 17 gradients (autograd's own slice nodes
    would each allocate and fill a zero [B, sum C] tensor)."""

    @staticmethod
    def forward(ctx, x, bounds):
        ctx.bounds, ctx.shape = bounds, tuple(x.shape)
        return tuple(x[:, a:b] for a, b in bounds)

    @staticmethod
    def backward(ctx, *grads):
        if any(g is None for g in grads):
            full = torch.zeros(ctx.shape, dtype=next(g for g in grads if g is not None).dtype, device=next(g for g in grads if g is not None).device)
            for (a, b), g in zip(ctx.bounds, grads):
                if g is not None:
                    full[:, a:b] = g
            return full, None
        return torch.cat(grads, dim=1), None


class ProjGroup:
    """`h += time_proj(temb) + text_proj(pooled)` of every ResBlock (unet.py:119-124) depends only on temb / pooled: with the 17
    weights of a kind ADJACENT in the parameter arena (UNet.arena_layout) they are one [sum Cout, K] operand, and the 34 tiny
    M = batch GEMMs of a forward (+ 34 data gradients, 34 weight gradients and the 32 accumulation adds of temb's / pooled's
    gradients in backward) become two Linear nodes over VIRTUAL parameters: leaf views of the flat master buffer whose
    gradient sink is the matching run of the gradient arena and whose prepared bf16 operand is the matching run of the AdamW
    shadow.  state_dict, the optimizer and the all-reduce never see them - they see the 68 real parameters, which are marked
    written (and reported to the data-parallel reducer) when the group's gradient lands."""

    def __init__(self, blocks, param_arena, grad_arena):
        self.ok = False
        self.blocks = list(blocks)
        pidx = {id(p): i for i, p in enumerate(param_arena.params)}
        self.pa, self.ga = param_arena, grad_arena
        self.virtual = []                       # (w_all, b_all) per kind
        self.bounds, off = [], 0
        for blk in self.blocks:
            self.bounds.append((off, off + blk.out_channels))
            off += blk.out_channels
        self.width = off
        self.members = []
        for kind in ("time_proj", "text_proj"):
            ws, bs = [getattr(b, kind).weight for b in self.blocks], [getattr(b, kind).bias for b in self.blocks]
            if any(id(t) not in pidx for t in ws + bs):
                return
            wi, bi = tuple(pidx[id(t)] for t in ws), tuple(pidx[id(t)] for t in bs)
            for idx in (wi, bi):                # one contiguous run each, in block order, in BOTH arenas
                for a, b in zip(idx[:-1], idx[1:]):
                    if param_arena.offsets[b] != param_arena.offsets[a] + param_arena.params[a].numel() or grad_arena.offsets[b] != param_arena.offsets[b]:
                        return
            K = ws[0].shape[1]
            ow, ob = param_arena.offsets[wi[0]], param_arena.offsets[bi[0]]
            w_all = param_arena.flat[ow:ow + self.width * K].view(self.width, K).requires_grad_(True)
            b_all = param_arena.flat[ob:ob + self.width].requires_grad_(True)
            gw = grad_arena.flat[ow:ow + self.width * K].view(self.width, K)
            gb = grad_arena.flat[ob:ob + self.width]
            for virt, view, idx in ((w_all, gw, wi), (b_all, gb, bi)):
                ents = [grad_arena.entries[i] for i in idx]
                ve = GradSink.register(virt, view, -1, on_ready=(lambda _i, ents=ents: [GradSink.done(e) for e in ents]), owner=grad_arena)
                grad_arena.extra_entries.append(ve)
                ParamShadow.register(virt, param_arena, idx)
            self.virtual.append((w_all, b_all))
            self.members.append(ws + bs)
        self._versions = self._member_versions()
        self.ok = True

    def _member_versions(self):
        return tuple(p._version for m in self.members for p in m)

    def usable(self):
        """Both arenas still own the parameters, and a member changed behind the optimizer's back (load_state_dict, an in-place
        torch op: its own version counter, which the virtual views do not share) drops the group's prepared operands."""
        if not self.ok or self.pa._displaced_by is not None or self.ga._displaced:
            return False
        v = self._member_versions()
        if v != self._versions:
            self._versions = v
            WeightCache.drop([t for pair in self.virtual for t in pair])
        return True

    def release(self):
        WeightCache.drop([t for pair in self.virtual for t in pair])
        for pair in self.virtual:
            for t in pair:
                e = GradSink._map.pop(id(t), None)
                if e is not None and e in self.ga.extra_entries:
                    self.ga.extra_entries.remove(e)
                ParamShadow._map.pop(id(t), None)
        self.ok = False

    def rowadds(self, temb, pooled):
        """The 17 per-sample additive vectors [B, Cout_k] (views of one [B, sum Cout] result)."""
        (wt, bt), (wx, bx) = self.virtual
        ra = linear(temb, wt, bt)
        ra = linear(pooled, wx, bx, residual=ra)
        if torch.is_grad_enabled() and ra.requires_grad:
            return _SplitColsFn.apply(ra, tuple(self.bounds))
        return tuple(ra[:, a:b] for a, b in self.bounds)


# ---------------------------------------------------------------------------
# GroupNorm (+SiLU)
# ---------------------------------------------------------------------------
class _GroupNormFn(torch.autograd.Function):
    """y = GroupNorm(x) [+SiLU]; with `passthrough` the node has a second output that IS x (for the consumer that
    bypasses the norm - ResBlock skip, attention residual): backward then receives both gradients and adds the
    bypass one inside the GroupNorm-backward kernel (psg_groupnorm_bwd_res) instead of autograd running a separate
    accumulation pass over the activation gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, silu, passthrough=False):
        lib = _lib_for(x)
        dtype = x.dtype
        xr, ldx = _rows(x)
        B, Cc = x.shape[0], x.shape[-1]
        HW = x.numel() // (B * Cc)
        y = torch.empty(x.shape, dtype=dtype, device=x.device)
        stats = torch.empty((2, B * groups), dtype=torch.float32, device=x.device)
        ws = _lib.workspace(lib.psg_groupnorm_fwd_workspace_bytes(B, groups), x.device)
        check(lib.psg_groupnorm_fwd(ptr(xr), ldx, ptr(y), Cc, ptr(gamma), ptr(beta), ptr(stats[0]), ptr(stats[1]), B, HW, Cc, groups,
                                    float(eps), int(silu), dtype_code(dtype), ptr(ws), stream_ptr()), "psg_groupnorm_fwd")
        ctx.save_for_backward(xr, gamma, beta, stats)
        ctx.gamma_param, ctx.beta_param = gamma, beta
        ctx.meta = (B, HW, Cc, groups, silu, ldx, tuple(x.shape))
        if passthrough:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dpass=None):
        xr, gamma, beta, stats = ctx.saved_tensors
        B, HW, Cc, groups, silu, ldx, shape = ctx.meta
        if dy is None:                               # only the bypass consumer produced a gradient
            return dpass, None, None, None, None, None, None
        lib = _lib_for(dy)
        dtype = dy.dtype
        dyr, lddy = _rows(dy)
        dres, lddres = (None, 0)
        if dpass is not None:
            dres, lddres = _rows(dpass if dpass.dtype == dtype else dpass.to(dtype))
        dx = torch.empty(shape, dtype=dtype, device=dy.device)
        # The kernel always produces both parameter gradients, so this node does not gate on needs_input_grad as LayerNorm and
        # BertEmbed do: a frozen gamma / beta that has a sink entry is written and reported ready too (as it always was).
        ag = _AffineGrads(ctx.gamma_param, ctx.beta_param, True, True)
        ws = _lib.workspace(lib.psg_groupnorm_bwd_workspace_bytes(B, Cc), dy.device)
        check(lib.psg_groupnorm_bwd_res(ptr(dyr), lddy, ptr(xr), ldx, ptr(gamma), ptr(beta), ptr(stats[0]), ptr(stats[1]), ptr(dres), lddres,
                                        ptr(dx), Cc, ptr(ag.dgamma), ptr(ag.dbeta), B, HW, Cc, groups, int(silu), int(ag.accumulate),
                                        dtype_code(dtype), ptr(ws), stream_ptr()), "psg_groupnorm_bwd_res")
        dg, db = ag.finish()
        return dx, dg, db, None, None, None, None


def group_norm(x, gamma, beta, groups, eps=1e-5, silu=False):
    """nn.GroupNorm (+F.silu) on channels-last [B, ..., C]: unet.py:115,127,214,231,397."""
    return _GroupNormFn.apply(x, gamma, beta, groups, eps, silu)


def group_norm_split(x, gamma, beta, groups, eps=1e-5, silu=False):
    """(GroupNorm(x), x): use the second result wherever x itself is consumed next to the norm (skip / residual
    paths), so the two gradients meet inside the GroupNorm-backward kernel (see _GroupNormFn)."""
    if not (_GN_SPLIT and torch.is_grad_enabled() and x.requires_grad):
        return _GroupNormFn.apply(x, gamma, beta, groups, eps, silu), x
    return _GroupNormFn.apply(x, gamma, beta, groups, eps, silu, True)


# ---------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------
def layer_norm_fwd(x, gamma, beta, eps, residual=None, out_dtype=None):
    """The psg_layernorm launch of `layer_norm` and of the frozen text encoder: (y, xr, ldx, rr, ldr) - the result in
    `out_dtype` (x's by default) and the row-addressed operands, which are all a backward needs."""
    lib = _lib_for(x)
    N = x.shape[-1]
    xr, ldx = _rows(x)
    rr, ldr = _rows(residual) if residual is not None else (None, 0)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    check(lib.psg_layernorm(ptr(xr), ldx, ptr(rr), ldr, ptr(y), N, ptr(gamma), ptr(beta), x.numel() // N, N, float(eps), dtype_code(x.dtype),
                            dtype_code(out_dtype), stream_ptr()), "psg_layernorm")
    return y, xr, ldx, rr, ldr


class _LayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x [+ residual]) * gamma + beta over the last dimension: psg_layernorm / psg_layernorm_bwd.  Only the
    inputs are saved (the backward recomputes the statistics); the one dz serves x and the residual."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, residual, out_dtype):
        y, xr, ldx, rr, ldr = layer_norm_fwd(x, gamma, beta, eps, residual, out_dtype)
        ctx.save_for_backward(xr, rr, gamma)
        ctx.gamma_param, ctx.beta_param = gamma, beta
        ctx.meta = (x.numel() // x.shape[-1], x.shape[-1], float(eps), ldx, ldr, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        xr, rr, gamma = ctx.saved_tensors
        rows, N, eps, ldx, ldr, shape = ctx.meta
        lib = _lib_for(dy)
        dyr, lddy = _rows(dy)
        dz = torch.empty(shape, dtype=xr.dtype, device=dy.device)
        want_g, want_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        ag = _AffineGrads(ctx.gamma_param, ctx.beta_param, want_g, want_b)
        need = lib.psg_layernorm_bwd_workspace_bytes(rows, N) if (want_g or want_b) else 0
        ws = _lib.workspace(need, dy.device) if need else None
        check(lib.psg_layernorm_bwd(ptr(xr), ldx, ptr(rr), ldr, ptr(dyr), lddy, ptr(gamma), ptr(dz), N, ptr(ag.dgamma), ptr(ag.dbeta),
                                    int(ag.accumulate), rows, N, eps, dtype_code(xr.dtype), dtype_code(dy.dtype), ptr(ws),
                                    ws.numel() if ws is not None else 0, stream_ptr()), "psg_layernorm_bwd")
        dg, db = ag.finish()
        need_x = ctx.needs_input_grad[0]
        need_r = rr is not None and ctx.needs_input_grad[4]
        return (dz if need_x else None), dg, db, None, (dz if need_r else None), None


def layer_norm(x, weight, bias, eps, residual=None, out_dtype=None):
    """nn.LayerNorm over the last dimension of x [..., N] (+ a residual added first: BERT's post-LN), fp32 parameters;
    `out_dtype`: the result's dtype (x's by default).  The forward launch is `layer_norm_fwd`, the frozen text encoder's."""
    return _LayerNormFn.apply(x, weight, bias, eps, residual, out_dtype)


# ---------------------------------------------------------------------------
# BertEmbeddings
# ---------------------------------------------------------------------------
_pos_index = {}


def _position_runs(B, S, device):
    """(key, perm) of the position table's scatter: key = t % S of the rows t = b*S + s in ascending order, ties in ascending b."""
    k = (B, S, device)
    if k not in _pos_index:
        j = torch.arange(B * S, dtype=torch.int64, device=device)
        _pos_index[k] = (j // B, (j % B) * S + j // B)
    return _pos_index[k]


def bert_embed_fwd(ids, type_ids, word, pos, typ, gamma, beta, eps, dtype, drop_p=0.0, seed=0):
    """The launches of `bert_embed` and of the frozen text encoder: psg_bert_embed_ln over token ids [B, S] -> [B*S, N] rows
    in `dtype`, then (drop_p > 0) psg_dropout_apply in place with the mask drawn from `seed`."""
    lib = _lib_for(word)
    B, S = ids.shape
    V, N = word.shape
    y = torch.empty((B * S, N), dtype=dtype, device=word.device)
    check(lib.psg_bert_embed_ln(ptr(ids), ptr(type_ids), ptr(word), ptr(pos), ptr(typ), ptr(gamma), ptr(beta), ptr(y), N, B, S, N, V,
                                pos.shape[0], typ.shape[0], float(eps), dtype_code(dtype), stream_ptr()), "psg_bert_embed_ln")
    if drop_p > 0:
        check(lib.psg_dropout_apply(ptr(y), N, ptr(y), N, B * S, N, drop_p, seed, 1.0 / (1.0 - drop_p), dtype_code(dtype), stream_ptr()),
              "psg_dropout_apply")
    return y


class _BertEmbedFn(torch.autograd.Function):
    """y = dropout(LayerNorm(word[ids] + type[type_ids] + pos[s])): `bert_embed_fwd`, and its backward psg_bert_embed_ln_bwd +
    one psg_embed_scatter per table whose gradient is wanted.  Only the ids are kept; the keys are sorted on the device
    (integer plumbing), nothing synchronises with the host."""

    @staticmethod
    def forward(ctx, ids, type_ids, word, pos, typ, gamma, beta, eps, pad_id, dtype, drop_p, seed):
        y = bert_embed_fwd(ids, type_ids, word, pos, typ, gamma, beta, eps, dtype, drop_p, seed)
        ctx.save_for_backward(ids, type_ids, word, pos, typ, gamma)
        ctx.params = (word, pos, typ, gamma, beta)
        ctx.meta = (*ids.shape, float(eps), int(pad_id), float(drop_p), seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        ids, type_ids, word, pos, typ, gamma = ctx.saved_tensors
        B, S, eps, pad_id, drop_p, seed = ctx.meta
        p_word, p_pos, p_typ, p_gamma, p_beta = ctx.params
        V, N = word.shape
        rows = B * S
        lib = _lib_for(dy)
        dev = dy.device
        dyr, lddy = _rows(dy)
        if drop_p > 0:
            g = torch.empty((rows, N), dtype=dy.dtype, device=dev)
            check(lib.psg_dropout_apply(ptr(dyr), lddy, ptr(g), N, rows, N, drop_p, seed, 1.0 / (1.0 - drop_p), dtype_code(dy.dtype), stream_ptr()),
                  "psg_dropout_apply")
            dyr, lddy = g, N
        want_w, want_p, want_t, want_g, want_b = ctx.needs_input_grad[2:7]
        need = max(lib.psg_bert_embed_ln_bwd_workspace_bytes(rows, N) if (want_g or want_b) else 0,
                   lib.psg_embed_scatter_workspace_bytes(rows, N) if (want_w or want_p or want_t) else 0)
        ws = _lib.workspace(need, dev) if need else None
        nws = ws.numel() if ws is not None else 0
        ag = _AffineGrads(p_gamma, p_beta, want_g, want_b)
        dz = torch.empty((rows, N), dtype=torch.float32, device=dev)
        check(lib.psg_bert_embed_ln_bwd(ptr(ids), ptr(type_ids), ptr(word), ptr(pos), ptr(typ), ptr(gamma), ptr(dyr), lddy, ptr(dz),
                                        ptr(ag.dgamma), ptr(ag.dbeta), int(ag.accumulate), B, S, N, V, pos.shape[0], typ.shape[0], eps,
                                        dtype_code(dy.dtype), ptr(ws), nws, stream_ptr()), "psg_bert_embed_ln_bwd")

        def scatter(param, key, perm, skip):
            out, acc, e = _param_out(param)
            if not out.is_contiguous():
                raise _lib.PsgError("bert_embed: the gradient of an embedding table must be a contiguous [V, N] tensor")
            check(lib.psg_embed_scatter(ptr(dz), N, ptr(key), ptr(perm), ptr(out), rows, N, param.shape[0], skip, int(acc), ptr(ws), nws,
                                        stream_ptr()), "psg_embed_scatter")
            return _param_ret(out, e)

        dw = dp = dt = None
        if want_w:
            dw = scatter(p_word, *torch.sort(ids.view(-1), stable=True), pad_id)
        if want_p:
            dp = scatter(p_pos, *_position_runs(B, S, dev), -1)
        if want_t:
            if type_ids is None:                     # every row is type 0: one run in row order
                order = _position_runs(1, rows, dev)[1]
                dt = scatter(p_typ, torch.zeros_like(order), order, -1)
            else:
                dt = scatter(p_typ, *torch.sort(type_ids.view(-1), stable=True), -1)
        dg, db = ag.finish()                         # (after the scatters: the tables are reported ready before gamma and beta)
        return None, None, dw, dp, dt, dg, db, None, None, None, None, None


def bert_embed(ids, type_ids, word, pos, typ, gamma, beta, eps, pad_id=0, dtype=torch.float32, drop_p=0.0, seed=0):
    """transformers' BertEmbeddings over token ids [B, S] (int64, contiguous; type_ids the same or None) -> [B*S, N] rows in
    `dtype`, with the embedding dropout drawn from `seed` when drop_p > 0; fp32 tables and LayerNorm parameters, whose gradients
    the backward produces (row `pad_id` of the word table gets none, as nn.Embedding's padding_idx)."""
    return _BertEmbedFn.apply(ids, type_ids, word, pos, typ, gamma, beta, eps, pad_id, dtype, drop_p, seed)


# ---------------------------------------------------------------------------
# attention core
# ---------------------------------------------------------------------------
def _attn_operands(q_src, kv_src, heads, rowed=False):
    """The operands of the attention entries for packed projections - self (kv_src None): q_src [B,L,3E] holds the q | k | v
    columns; cross: q_src [B,L,E] and kv_src [B,S,2E] with the k | v columns.  Returns (qr, kvr, io, dims, E): the
    row-addressed tensors behind the pointers, io = (q, ldq, k, ldk, v, ldk) and dims = (B, heads, L, S, d), both in the
    entries' argument order.  `rowed`: the tensors are results of `_rows` already (a backward's saved inputs) or freshly
    allocated (its gradient outputs, packed the same way) and are taken as they are - no second check, and no copy, which
    for an output would swallow the result."""
    qr, ldq = (q_src, q_src.stride(-2)) if rowed else _rows(q_src)
    B, L = q_src.shape[0], q_src.shape[1]
    esz = qr.element_size()
    if kv_src is None:
        E, S, kvr, ldk = q_src.shape[-1] // 3, L, None, ldq
        kp = qr.data_ptr() + E * esz
    else:
        E, S = q_src.shape[-1], kv_src.shape[1]
        kvr, ldk = (kv_src, kv_src.stride(-2)) if rowed else _rows(kv_src)
        kp = kvr.data_ptr()
    return qr, kvr, (qr.data_ptr(), ldq, kp, ldk, kp + E * esz, ldk), (B, heads, L, S, E // heads), E


def attention_fwd(q_src, kv_src, heads, drop_p=0.0, seed=0, kv_len=None, want_lse=True):
    """The forward launch of every attention path: (o [B,L,E], lse, qr, kvr) - the result, the log-sum-exp and the row-addressed
    inputs, which are what a backward saves.  psg_attn_fwd; with `kv_len` (int32 [B] on the device: the keys of sample b end at kv_len[b])
    psg_attn_fwd_varlen_train, or - `want_lse` False, nothing kept for a backward, no dropout - psg_attn_fwd_varlen."""
    lib = _lib_for(q_src)
    dtype = q_src.dtype
    qr, kvr, io, dims, E = _attn_operands(q_src, kv_src, heads)
    B, _, L, _, d = dims
    o = torch.empty((B, L, E), dtype=dtype, device=q_src.device)
    lse = torch.empty((B, heads, L), dtype=torch.float32, device=q_src.device) if want_lse else None
    args = (*io, ptr(o), E, ptr(lse), *dims, float(d) ** -0.5, float(drop_p), int(seed), dtype_code(dtype))
    if kv_len is None:
        check(lib.psg_attn_fwd(*args, stream_ptr()), "psg_attn_fwd")
    elif want_lse:
        check(lib.psg_attn_fwd_varlen_train(*args, ptr(kv_len), stream_ptr()), "psg_attn_fwd_varlen_train")
    else:
        check(lib.psg_attn_fwd_varlen(*args, ptr(kv_len), stream_ptr()), "psg_attn_fwd_varlen")
    return o, lse, qr, kvr


class _AttnFn(torch.autograd.Function):
    """softmax((q/sqrt(d)) k^T) v for packed projections.  self: qkv [B,L,3E]; cross: q [B,L,E], kv [B,S,2E].
    With `kv_len` (int32 [B] on the device) the keys of sample b end at kv_len[b]: psg_attn_fwd_varlen_train / psg_attn_bwd_varlen."""

    @staticmethod
    def forward(ctx, q_src, kv_src, heads, drop_p, seed, kv_len=None):
        o, lse, qr, kvr = attention_fwd(q_src, kv_src, heads, drop_p, seed, kv_len)
        ctx.kv_len = kv_len
        ctx.save_for_backward(qr, kvr, o, lse)
        ctx.meta = (heads, drop_p, seed)
        return o

    @staticmethod
    def backward(ctx, do):
        qr, kvr, o, lse = ctx.saved_tensors
        heads, drop_p, seed = ctx.meta
        _, _, io, dims, _ = _attn_operands(qr, kvr, heads, True)
        B, _, L, _, d = dims
        lib = _lib_for(do)
        dtype = do.dtype
        dor, lddo = _rows(do)
        delta = torch.empty((B, heads, L), dtype=torch.float32, device=do.device)
        dqkv = torch.empty(qr.shape, dtype=dtype, device=do.device)
        dkv = None if kvr is None else torch.empty(kvr.shape, dtype=dtype, device=do.device)
        args = (*io, ptr(o), o.shape[-1], ptr(dor), lddo, ptr(lse), ptr(delta), *_attn_operands(dqkv, dkv, heads, True)[2], *dims,
                float(d) ** -0.5, float(drop_p), int(seed), dtype_code(dtype))
        if ctx.kv_len is None:
            check(lib.psg_attn_bwd(*args, stream_ptr()), "psg_attn_bwd")
        else:
            check(lib.psg_attn_bwd_varlen(*args, ptr(ctx.kv_len), stream_ptr()), "psg_attn_bwd_varlen")
        return dqkv, dkv, None, None, None, None


def attention_self(qkv, heads, drop_p=0.0, seed=0, kv_len=None):
    """Self-attention over packed qkv [B, L, 3E]; `kv_len` (int32 [B], device): the keys of sample b end at kv_len[b]."""
    if kv_len is None:
        return _AttnFn.apply(qkv, None, heads, drop_p, seed)
    return _AttnFn.apply(qkv, None, heads, drop_p, seed, kv_len)


def attention_cross(q, kv, heads, drop_p=0.0, seed=0):
    return _AttnFn.apply(q, kv, heads, drop_p, seed)


def attention_causal(qkv, heads):
    """Causal self-attention over packed qkv [B, L, 3E] (key s serves query l iff s <= l): psg_attn_fwd_causal, CLIP's text tower.
    Forward only - the text side of the loss is a constant: a qkv that asks for a gradient is refused."""
    if torch.is_grad_enabled() and qkv.requires_grad:
        raise _lib.PsgError("attention_causal is forward only: run it under torch.no_grad()")
    lib = _lib_for(qkv)
    qr, _, io, dims, E = _attn_operands(qkv, None, heads)      # qr: the tensor behind io's raw addresses (a copy when qkv's
    B, _, L, _, d = dims                                       # layout was irregular) - it must outlive the launch
    o = torch.empty((B, L, E), dtype=qkv.dtype, device=qkv.device)
    check(lib.psg_attn_fwd_causal(*io, ptr(o), E, None, *dims, float(d) ** -0.5, 0.0, 0, dtype_code(qkv.dtype), stream_ptr()),
          "psg_attn_fwd_causal")
    return o


class _AttnLongQFn(torch.autograd.Function):
    """Cross-attention of very many queries over few keys (the VAE decoder's text attention): q [B,L,E], kv [B,S,2E], no
    dropout.  Forward: psg_attn_fwd, the launch of `attention_cross`; backward: psg_attn_bwd_longq."""

    @staticmethod
    def forward(ctx, q_src, kv_src, heads):
        o, lse, qr, kvr = attention_fwd(q_src, kv_src, heads)
        ctx.save_for_backward(qr, kvr, o, lse)
        ctx.heads = heads
        return o

    @staticmethod
    def backward(ctx, do):
        qr, kvr, o, lse = ctx.saved_tensors
        heads = ctx.heads
        _, _, io, dims, E = _attn_operands(qr, kvr, heads, True)
        B, _, L, S, d = dims
        lib = _lib_for(do)
        dtype = do.dtype
        dor, lddo = _rows(do)
        delta = torch.empty((B, heads, L), dtype=torch.float32, device=do.device)
        dq = torch.empty((B, L, E), dtype=dtype, device=do.device)
        dkv = torch.empty((B, S, 2 * E), dtype=dtype, device=do.device)
        need = lib.psg_attn_bwd_longq_workspace_bytes(*dims)
        if need < 0:
            check(-1, "psg_attn_bwd_longq_workspace_bytes")
        ws = _lib.workspace(need, do.device)
        check(lib.psg_attn_bwd_longq(*io, ptr(o), E, ptr(dor), lddo, ptr(lse), ptr(delta), *_attn_operands(dq, dkv, heads, True)[2], *dims,
                                     float(d) ** -0.5, 0.0, 0, dtype_code(dtype), ptr(ws), ws.numel(), stream_ptr()), "psg_attn_bwd_longq")
        return dq, dkv, None


def attention_cross_longq(q, kv, heads):
    """`attention_cross` (no dropout) whose backward is the long-query kernel pair: vae_decoder.py:49-65 under stage 3."""
    return _AttnLongQFn.apply(q, kv, heads)


class _ReconLossFn(torch.autograd.Function):
    """(w_l1 * L1 + w_mse * MSE, L1, MSE) of fp32 tensors, each a mean over all elements: psg_recon_loss_f32.  The gradient is
    produced by the forward's own pass and belongs to the first of the three results."""

    @staticmethod
    def forward(ctx, pred, target, w_l1, w_mse):
        lib = _lib_for(pred)
        p, t = pred.detach().contiguous().float(), target.detach().to(pred.device).contiguous().float()
        if p.shape != t.shape:
            raise _lib.PsgError(f"recon_loss: shapes {tuple(p.shape)} and {tuple(t.shape)} differ")
        want = ctx.needs_input_grad[0]
        grad = torch.empty_like(p) if want else None
        out3 = torch.empty(3, dtype=torch.float32, device=p.device)
        ws = _lib.workspace(lib.psg_recon_loss_workspace_bytes(), p.device)
        check(lib.psg_recon_loss_f32(ptr(p), ptr(t), ptr(grad), ptr(out3), p.numel(), float(w_l1), float(w_mse), ptr(ws), stream_ptr()),
              "psg_recon_loss_f32")
        ctx.grad, ctx.shape = grad, tuple(pred.shape)
        return out3

    @staticmethod
    def backward(ctx, g):
        return ctx.grad.view(ctx.shape) * g[0], None, None, None


def recon_loss(pred, target, w_l1=1.0, w_mse=0.1):
    """final_trainer.py:425-440: (l1 + 0.1 * mse, l1, mse) as fp32 device scalars; one pass produces loss and gradient."""
    out3 = _ReconLossFn.apply(pred, target, w_l1, w_mse)
    return out3[0], out3[1].detach(), out3[2].detach()


# ---------------------------------------------------------------------------
# inference launches of frozen modules (the VAE, the text encoder, the perceptual loss's target side)
# ---------------------------------------------------------------------------
def prepared(cache, key, param_list, build):
    """Prepared (kernel-layout) weights of a frozen module, rebuilt when a parameter changes (version counters)."""
    stamp = tuple((p.data_ptr(), p._version) for p in param_list)
    ent = cache.get(key)
    if ent is None or ent[0] != stamp:
        ent = (stamp, build())
        cache[key] = ent
    return ent[1]


def conv_infer(x, wf, bias, Cin, Cout, ks=1, stride=1, pad=0, act=ACT_NONE, residual=None, out_dtype=None):
    """psg_conv_fwd on a prepared weight wf [Cout][Kpad], nothing kept for a backward.  x [B,H,W,Cin] channels-last (rows
    16-byte aligned) -> [B,Ho,Wo,Cout]; a 2-D x [M,Cin] is a Linear (ks = 1) -> [M,Cout]."""
    lib = _lib_for(x)
    xr, ldx = _rows(x)
    if x.dim() == 4:
        geom = _conv_geom(x, ks, stride, pad)
        out_shape = (geom[0], geom[3], geom[4], Cout)
    else:
        geom, out_shape = _linear_geom(x.shape[0]), (x.shape[0], Cout)
    y = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    res_r, ld_res = (None, 0) if residual is None else _rows(residual)
    _conv_launch(lib, x.dtype, xr, ldx, wf, 0, y, Cout, geom, Cin, Cout, bias=bias, residual=res_r, ld_res=ld_res, act=act)
    return y


def prep_weight(w, dtype, pad_in=0):
    """fp32 OIHW parameter -> prepared forward weight [O][Kpad] in `dtype`; optional zero padding of Cin."""
    lib = _lib_for(w)
    O, I, kh, kw = w.shape
    src = w.detach().float()
    if pad_in:
        src, I = torch.nn.functional.pad(src, (0, 0, 0, 0, 0, pad_in)), I + pad_in
    src = src.contiguous(memory_format=torch.channels_last)           # OHWI memory: the layout every kernel-side path takes
    code = dtype_code(dtype)
    kp = lib.psg_kpad(kh * kw * I, code)
    wf = torch.empty((O, kp), dtype=dtype, device=w.device)
    check(lib.psg_prep_weight(ptr(src), dtype_code(torch.float32), W_OHWI, ptr(wf), None, O, I, kh, code, stream_ptr()), "psg_prep_weight")
    return wf


# ---------------------------------------------------------------------------
# stage 1's loss around the VGG16 convolutions (src/models/losses.py)
# ---------------------------------------------------------------------------
class _MaxPoolFn(torch.autograd.Function):
    """nn.MaxPool2d(2, 2) on channels-last [B,H,W,C]: psg_maxpool2x2_fwd / _bwd.  Saved for backward: the winning taps
    (one byte per output element), written only when a gradient is wanted."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib_for(x)
        xr, ldx = _rows(x)
        B, Hi, Wi, Cc = x.shape
        y = torch.empty((B, Hi // 2, Wi // 2, Cc), dtype=x.dtype, device=x.device)
        tap = torch.empty(y.shape, dtype=torch.uint8, device=x.device) if ctx.needs_input_grad[0] else None
        check(lib.psg_maxpool2x2_fwd(ptr(xr), ldx, ptr(y), Cc, ptr(tap), B, Hi, Wi, Cc, dtype_code(x.dtype), stream_ptr()), "psg_maxpool2x2_fwd")
        ctx.tap, ctx.meta = tap, (B, Hi, Wi, Cc)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, Hi, Wi, Cc = ctx.meta
        lib = _lib_for(dy)
        dyr, lddy = _rows(dy)
        dx = torch.empty((B, Hi, Wi, Cc), dtype=dy.dtype, device=dy.device)
        check(lib.psg_maxpool2x2_bwd(ptr(dyr), lddy, ptr(ctx.tap), ptr(dx), Cc, B, Hi, Wi, Cc, dtype_code(dy.dtype), stream_ptr()),
              "psg_maxpool2x2_bwd")
        return dx


def max_pool2x2(x):
    """nn.MaxPool2d(kernel_size=2, stride=2) (floor; ties: the first tap) on channels-last [B,H,W,C]."""
    return _MaxPoolFn.apply(x)


class _ImagePrepFn(torch.autograd.Function):
    """fp32 NCHW image [B,3,H,W] -> normalised channels-last [B,Ho,Wo,8] in `dtype` (psg_image_prep_fwd): clamp(a img + b, 0, 1),
    bilinear resize to `size` if it differs, ImageNet normalisation; channels 3..7 zero.  Saved for backward: the image (the
    clamp mask is recomputed from it).  Backward: psg_image_prep_bwd, a gather with the forward's resize weights."""

    @staticmethod
    def forward(ctx, img, a, b, size, dtype):
        lib = _lib_for(img)
        if img.dim() != 4 or img.shape[1] != 3:
            raise _lib.PsgError(f"image_prep: expected a [B,3,H,W] image, got {tuple(img.shape)}")
        x = img.detach().contiguous().float()
        B, _, Hi, Wi = x.shape
        Ho, Wo = (Hi, Wi) if size is None else (int(size[0]), int(size[1]))
        y = torch.empty((B, Ho, Wo, 8), dtype=dtype, device=x.device)
        check(lib.psg_image_prep_fwd(ptr(x), ptr(y), 8, B, Hi, Wi, Ho, Wo, float(a), float(b), dtype_code(dtype), stream_ptr()),
              "psg_image_prep_fwd")
        ctx.img = x if ctx.needs_input_grad[0] else None
        ctx.meta = (B, Hi, Wi, Ho, Wo, float(a), float(b), tuple(img.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        B, Hi, Wi, Ho, Wo, a, b, shape = ctx.meta
        lib = _lib_for(dy)
        dyr, lddy = _rows(dy)
        dimg = torch.empty((B, 3, Hi, Wi), dtype=torch.float32, device=dy.device)
        check(lib.psg_image_prep_bwd(ptr(ctx.img), ptr(dyr), lddy, ptr(dimg), B, Hi, Wi, Ho, Wo, a, b, dtype_code(dy.dtype), stream_ptr()),
              "psg_image_prep_bwd")
        return dimg.view(shape), None, None, None, None


def image_prep(img, a=1.0, b=0.0, size=None, dtype=torch.float32):
    """losses.py:75-81 and :51-53 in one pass (see _ImagePrepFn); `size` None keeps the image's own size."""
    return _ImagePrepFn.apply(img, a, b, size, dtype)


class _FeatL1Fn(torch.autograd.Function):
    """(mean |a - b|, weight * mean |a - b|) of two feature maps as fp32 device scalars: psg_feat_l1.  The gradient with respect
    to `a` (weight * sign(a - b) / n, sign(0) = 0) is produced by the forward's own pass and belongs to the second result;
    `b` is a constant."""

    @staticmethod
    def forward(ctx, a, b, weight):
        lib = _lib_for(a)
        if a.shape != b.shape or a.dtype != b.dtype:
            raise _lib.PsgError(f"feature_l1: {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype} differ")
        ar, lda = _rows(a)
        br, ldb = _rows(b.detach())
        cols = ar.shape[-1]
        rows = ar.numel() // cols
        grad = torch.empty(a.shape, dtype=a.dtype, device=a.device) if ctx.needs_input_grad[0] else None
        out2 = torch.empty(2, dtype=torch.float32, device=a.device)
        ws = _lib.workspace(lib.psg_feat_l1_workspace_bytes(), a.device)
        check(lib.psg_feat_l1(ptr(ar), lda, ptr(br), ldb, ptr(grad), cols, ptr(out2), rows, cols, float(weight), dtype_code(a.dtype),
                              ptr(ws), ws.numel(), stream_ptr()), "psg_feat_l1")
        ctx.grad = grad
        return out2

    @staticmethod
    def backward(ctx, g):
        return (ctx.grad.float() * g[1]).to(ctx.grad.dtype), None, None      # fp32 product, one rounding (0.1 is not a bf16 number)


def feature_l1(a, b, weight=1.0):
    """weight * F.l1_loss(a, b) for feature maps [..., C] in the compute dtype (losses.py:89-90); the gradient reaches `a` only."""
    return _FeatL1Fn.apply(a, b, weight)[1]


class _KLFn(torch.autograd.Function):
    """losses.py:147-148: -0.5 * sum(1 + logvar - mu^2 - exp(logvar)) / numel as an fp32 device scalar (psg_kl_f32); both
    gradients come out of the forward's pass."""

    @staticmethod
    def forward(ctx, mu, logvar):
        lib = _lib_for(mu)
        if mu.shape != logvar.shape:
            raise _lib.PsgError(f"kl_loss: shapes {tuple(mu.shape)} and {tuple(logvar.shape)} differ")
        m, lv = mu.detach().contiguous().float(), logvar.detach().contiguous().float()
        dmu = torch.empty_like(m) if ctx.needs_input_grad[0] else None
        dlv = torch.empty_like(lv) if ctx.needs_input_grad[1] else None
        out = torch.empty(1, dtype=torch.float32, device=m.device)
        ws = _lib.workspace(lib.psg_kl_workspace_bytes(), m.device)
        check(lib.psg_kl_f32(ptr(m), ptr(lv), ptr(dmu), ptr(dlv), ptr(out), m.numel(), ptr(ws), ws.numel(), stream_ptr()), "psg_kl_f32")
        ctx.grads, ctx.shape = (dmu, dlv), tuple(mu.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        dmu, dlv = ctx.grads
        return (dmu.view(ctx.shape) * g[0] if dmu is not None else None), (dlv.view(ctx.shape) * g[0] if dlv is not None else None)


def kl_loss(mu, logvar):
    """The KL term of CombinedLoss (mean over all latent elements) as an fp32 device scalar."""
    return _KLFn.apply(mu, logvar)[0]


# ---------------------------------------------------------------------------
# stage 3's CLIP loss around the two towers (src/models/clip_loss.py)
# ---------------------------------------------------------------------------
class _ClipPrepFn(torch.autograd.Function):
    """fp32 NCHW image [B,3,H,H] -> the vision tower's patch rows [B, (size/patch)^2, 3*patch^2] in `dtype` (psg_clip_prep_fwd):
    a img + b, antialiased bicubic resize to `size` if H differs, CLIP normalisation.  Nothing is saved: the pass is linear in
    the image.  Backward: psg_clip_prep_bwd, a gather with the forward's weights."""

    @staticmethod
    def forward(ctx, img, a, b, size, patch, dtype):
        lib = _lib_for(img)
        if img.dim() != 4 or img.shape[1] != 3:
            raise _lib.PsgError(f"clip_prep: expected a [B,3,H,W] image, got {tuple(img.shape)}")
        x = img.detach().contiguous().float()
        B, _, Hi, Wi = x.shape
        size, patch = int(size), int(patch)
        cols = 3 * patch * patch
        y = torch.empty((B, (size // max(patch, 1)) ** 2, cols), dtype=dtype, device=x.device)
        check(lib.psg_clip_prep_fwd(ptr(x), ptr(y), cols, B, Hi, Wi, size, patch, float(a), float(b), dtype_code(dtype), stream_ptr()),
              "psg_clip_prep_fwd")
        ctx.meta = (B, Hi, Wi, size, patch, float(a), tuple(img.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        B, Hi, Wi, size, patch, a, shape = ctx.meta
        lib = _lib_for(dy)
        dyr, lddy = _rows(dy)
        dimg = torch.empty((B, 3, Hi, Wi), dtype=torch.float32, device=dy.device)
        check(lib.psg_clip_prep_bwd(ptr(dyr), lddy, ptr(dimg), B, Hi, Wi, size, patch, a, dtype_code(dy.dtype), stream_ptr()),
              "psg_clip_prep_bwd")
        return dimg.view(shape), None, None, None, None, None


def clip_prep(img, size, patch, a=0.5, b=0.5, dtype=torch.float32):
    """clip_loss.py:52,55 for the image in one pass (see _ClipPrepFn): square images no larger than `size`."""
    return _ClipPrepFn.apply(img, a, b, size, patch, dtype)


class _CosineLossFn(torch.autograd.Function):
    """-mean_b(normalize(u[b]) . normalize(v[b])) of u, v [B, D] as an fp32 device tensor [1]: psg_cosine_loss.  The gradient
    with respect to `u` is produced by the forward's own pass; `v` is a constant."""

    @staticmethod
    def forward(ctx, u, v):
        lib = _lib_for(u)
        if u.dim() != 2 or u.shape != v.shape or u.dtype != v.dtype:
            raise _lib.PsgError(f"cosine_loss: {tuple(u.shape)} {u.dtype} and {tuple(v.shape)} {v.dtype} must be equal [B, D] operands")
        ur, ldu = _rows(u)
        vr, ldv = _rows(v.detach())
        B, D = u.shape
        du = torch.empty((B, D), dtype=u.dtype, device=u.device) if ctx.needs_input_grad[0] else None
        out = torch.empty(1, dtype=torch.float32, device=u.device)
        check(lib.psg_cosine_loss(ptr(ur), ldu, ptr(vr), ldv, ptr(du), D, ptr(out), B, D, dtype_code(u.dtype), stream_ptr()), "psg_cosine_loss")
        ctx.du = du
        return out

    @staticmethod
    def backward(ctx, g):
        return (ctx.du.float() * g[0]).to(ctx.du.dtype), None


def cosine_loss(u, v):
    """clip_loss.py:60-67: -(F.normalize(u) * F.normalize(v)).sum(-1).mean() as an fp32 device scalar; the gradient reaches `u` only."""
    return _CosineLossFn.apply(u, v.detach())[0]


# ---------------------------------------------------------------------------
# small ops
# ---------------------------------------------------------------------------
class _UpsampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo):
        lib = _lib_for(x)
        xr, ldx = _rows(x)
        B, Hi, Wi, Cc = x.shape
        y = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
        check(lib.psg_upsample_bilinear_fwd(ptr(xr), ldx, ptr(y), Cc, B, Hi, Wi, Ho, Wo, Cc, dtype_code(x.dtype), stream_ptr()),
              "psg_upsample_bilinear_fwd")
        ctx.meta = (B, Hi, Wi, Ho, Wo, Cc)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, Hi, Wi, Ho, Wo, Cc = ctx.meta
        lib = _lib_for(dy)
        dyr, lddy = _rows(dy)
        dx = torch.empty((B, Hi, Wi, Cc), dtype=dy.dtype, device=dy.device)
        check(lib.psg_upsample_bilinear_bwd(ptr(dyr), lddy, ptr(dx), Cc, B, Hi, Wi, Ho, Wo, Cc, dtype_code(dy.dtype), stream_ptr()),
              "psg_upsample_bilinear_bwd")
        return dx, None, None


def upsample_bilinear(x, size):
    """nn.Upsample(size, mode='bilinear', align_corners=False) — unet.py:365,375,385."""
    return _UpsampleFn.apply(x, int(size[0]), int(size[1]))


def nhwc_rows_to_nchw(xr, ldx, C):
    """The first C columns of the rows of xr [B,H,W,>=C] (row stride ldx, compute dtype) -> fp32 [B,C,H,W]: psg_nhwc_to_nchw."""
    lib = _lib_for(xr)
    B, H, W = xr.shape[0], xr.shape[1], xr.shape[2]
    y = torch.empty((B, C, H, W), dtype=torch.float32, device=xr.device)
    check(lib.psg_nhwc_to_nchw(ptr(xr), ldx, ptr(y), B, C, H * W, dtype_code(xr.dtype), stream_ptr()), "psg_nhwc_to_nchw")
    return y


def nchw_to_nhwc(x, dtype, width=None):
    """[B,C,H,W] fp32 -> [B,H,W,C] compute dtype (network input; no gradient): psg_nchw_to_nhwc.  `width` > C: rows of that
    many columns, the padding columns zero."""
    lib = _lib_for(x)
    xc = x.detach().contiguous().float()
    B, Cc, H, W = xc.shape
    width = Cc if width is None else width
    y = (torch.empty if width == Cc else torch.zeros)((B, H, W, width), dtype=dtype, device=x.device)
    check(lib.psg_nchw_to_nhwc(ptr(xc), ptr(y), width, B, Cc, H * W, dtype_code(dtype), stream_ptr()), "psg_nchw_to_nhwc")
    return y


class _ToNCHWFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.dtype = x.dtype
        return nhwc_rows_to_nchw(*_rows(x), x.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        return nchw_to_nhwc(dy, ctx.dtype)


def nhwc_to_nchw(x):
    """channels-last compute dtype -> the reference's NCHW fp32 boundary layout (differentiable)."""
    return _ToNCHWFn.apply(x)


class _ToNHWCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        return nchw_to_nhwc(x, dtype)

    @staticmethod
    def backward(ctx, dy):
        with torch.no_grad():
            return nhwc_to_nchw(dy), None


def nchw_to_nhwc_grad(x, dtype):
    """`nchw_to_nhwc` with the gradient carried back to the fp32 NCHW input (the VAE decoder's latent)."""
    return _ToNHWCFn.apply(x, dtype)


class _ImageOutFn(torch.autograd.Function):
    """The first `cout` of the C columns of y [B,H,W,C] -> fp32 [B,cout,H,W] (the decoder's image: 3 channels computed in padded
    columns); backward writes zeros into the padding columns."""

    @staticmethod
    def forward(ctx, y, cout):
        ctx.meta = (y.shape[-1], y.dtype)
        return nhwc_rows_to_nchw(y, y.shape[-1], cout)

    @staticmethod
    def backward(ctx, dimg):
        Cc, dtype = ctx.meta
        return nchw_to_nhwc(dimg, dtype, width=Cc), None


def image_out(y, cout):
    return _ImageOutFn.apply(y.contiguous(), cout)


class _PadRowsFn(torch.autograd.Function):
    """param [n, ...] fp32 -> [n + extra, ...] with zero rows appended (the decoder's trainable 3-channel image conv computed
    in 8 output columns, vae_decoder.py:175).  Backward takes the first n rows of the padded gradient: the padding rows
    contribute nothing to the output and receive nothing.  The weight-gradient kernel writes the PADDED shape, which a sink
    entry of the parameter's own shape cannot take, so a registered parameter is delivered through one small copy (a few
    hundred values) into its GradSink view - written on first use in a step, accumulated afterwards, as the kernels do."""

    @staticmethod
    def forward(ctx, param, extra):
        ctx.param, ctx.n = param, param.shape[0]
        out = torch.zeros((param.shape[0] + extra,) + tuple(param.shape[1:]), dtype=torch.float32, device=param.device)
        out[:ctx.n].copy_(param.detach())
        return out

    @staticmethod
    def backward(ctx, g):
        own = g[:ctx.n]
        e = GradSink.get(ctx.param)
        if e is None:
            return own.clone(), None
        e.view.add_(own) if e.written else e.view.copy_(own)
        GradSink.done(e)
        return None, None


def pad_rows(param, extra):
    """`param` with `extra` zero rows appended along dim 0, differentiable with respect to `param` (see `_PadRowsFn`)."""
    return _PadRowsFn.apply(param, extra)


def text_pool(text, dtype):
    """AdaptiveAvgPool1d(1) over tokens (unet.py:445) + compute-dtype copy of the tokens."""
    lib = _lib_for(text)
    tc = text.detach().contiguous().float()
    B, S, D = tc.shape
    pooled = torch.empty((B, D), dtype=dtype, device=text.device)
    cast = torch.empty((B, S, D), dtype=dtype, device=text.device)
    check(lib.psg_text_pool(ptr(tc), ptr(pooled), D, ptr(cast), B, S, D, dtype_code(dtype), stream_ptr()), "psg_text_pool")
    return pooled, cast


def timestep_sinusoid(t, coeff, dtype):
    """cat[sin(t*coeff), cos(t*coeff)] (unet.py:47-50)."""
    lib = _lib_for(coeff)
    tt = t.detach().to(device=coeff.device, dtype=torch.int64).contiguous()
    B, half = tt.shape[0], coeff.shape[0]
    out = torch.empty((B, 2 * half), dtype=dtype, device=coeff.device)
    check(lib.psg_timestep_sinusoid(ptr(tt), ptr(coeff.detach().float().contiguous()), ptr(out), 2 * half, B, half, dtype_code(dtype),
                                    stream_ptr()), "psg_timestep_sinusoid")
    return out
