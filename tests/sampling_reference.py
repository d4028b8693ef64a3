"""numpy restatement of the neighbour sampler's definition (include/hcspmm.h), written from the definition and not from the
kernel: the key, the selection and the scan.

  fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16              (uint32 arithmetic)
  key(e, seed) = fmix32(fmix32((uint32)e * 0x9E3779B1 + (uint32)seed) + (uint32)(seed >> 32))       seed: uint64, e: CSR position

A row with deg <= fanout keeps all its entries; a longer one keeps the `fanout` entries with the smallest keys; kept entries
stay in ascending e.  row_pointers_s is the exclusive scan of min(deg, fanout)."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & _M32  # 32-bit values in 64-bit lanes: a product of two of them cannot wrap
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def keys(e, seed):
    """key(e, seed) for an array of CSR positions -> uint64 array of 32-bit values"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    e32 = np.asarray(e, dtype=np.int64).astype(np.uint64) & _M32
    inner = fmix32(((e32 * np.uint64(0x9E3779B1)) & _M32) + np.uint64(seed & 0xFFFFFFFF))
    return fmix32(inner + np.uint64(seed >> 32))


def sample_row_pointers(row_pointers, fanout):
    deg = np.diff(np.asarray(row_pointers, dtype=np.int64))
    return np.concatenate([[0], np.cumsum(np.minimum(deg, int(fanout)))]).astype(np.int32)


def sample_neighbors(row_pointers, column_index, fanout, seed):
    """-> (row_pointers_s, column_index_s, entry_index_s), int32"""
    rp = np.asarray(row_pointers, dtype=np.int64)
    col = np.asarray(column_index)
    fanout = int(fanout)
    rp_s = sample_row_pointers(rp, fanout)
    deg = np.diff(rp)
    eid_s = np.empty(int(rp_s[-1]), dtype=np.int64)
    # rows that keep everything
    rows = np.repeat(np.arange(len(deg)), deg)
    e = np.arange(len(rows), dtype=np.int64)
    through = deg[rows] <= fanout
    eid_s[rp_s[rows[through]] + (e[through] - rp[rows[through]])] = e[through]
    # longer rows: the `fanout` smallest keys, back in ascending e
    for r in np.nonzero(deg > fanout)[0]:
        er = np.arange(rp[r], rp[r + 1], dtype=np.int64)
        k = keys(er, seed)
        order = np.argsort(k, kind="stable")
        assert len(np.unique(k)) == len(k)  # a bijection of e: no ties
        eid_s[rp_s[r]:rp_s[r + 1]] = np.sort(er[order[:fanout]])
    return rp_s, col[eid_s].astype(np.int32), eid_s.astype(np.int32)
