"""Integer-only restatement of the kernels' stateless dropout hash (csrc/psg_common.h: mix32, drop_hash_pair, drop_thresh,
drop_keep) - test infrastructure shared by tests/attn_ref.py (attention masks) and tests/gemm_ref.py (conv epilogue masks).
Nothing here reads a mask off a launch: the masks are recomputed from the seed and the element index alone."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def mix32(h):
    """psg_common.h mix32 (murmur3's 32-bit finaliser) on an array of values < 2^32, in integers only."""
    h = np.asarray(h, dtype=np.uint64) & _M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def drop_hash_pair(seed, pair):
    """psg_common.h drop_hash_pair: one 32-bit hash for the elements 2 pair, 2 pair + 1.  seed: int < 2^64; pair: uint64 array."""
    pair = np.asarray(pair, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = pair & _M32, pair >> np.uint64(32)
    t = ((hi * np.uint64(0x85EBCA77)) & _M32) ^ np.uint64(seed >> 32)
    return mix32((((lo * np.uint64(0x9E3779B1)) & _M32) + np.uint64(seed & 0xFFFFFFFF) + t) & _M32)


def drop_thresh(p):
    """psg_common.h drop_thresh: floor(p 2^32) of the fp32 rate, saturated."""
    t = float(np.float32(p)) * 4294967296.0
    return int(min(max(t, 0.0), 4294967295.0))


def keep_flat(seed, idx, p):
    """psg_common.h drop_keep on an array of flat element indices: element idx shares the hash of pair idx >> 1 and takes
    its low (even idx) or high (odd idx) 16 bits, kept when >= thresh >> 16.  All True at p = 0."""
    idx = np.asarray(idx, dtype=np.uint64)
    if not p > 0.0:
        return np.ones(idx.shape, dtype=bool)
    hh = drop_hash_pair(seed, idx >> np.uint64(1))
    half = np.where((idx & np.uint64(1)) == 1, hh >> np.uint64(16), hh & np.uint64(0xFFFF))
    return half >= np.uint64(drop_thresh(p) >> 16)
