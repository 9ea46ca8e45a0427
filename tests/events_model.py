"""Numpy model of the event path as include/qldpc_hip.h specifies it (qldpc_circuit_plan_decode_events): the record format, the layout gather and the
prediction.  No library import: the tests pin the GPU kernels and the library's own pack helpers to it bit for bit."""
import numpy as np


def pack(bits):
    """0 / 1 array [count, n_bits] -> records uint8[count, ceil(n_bits / 8)]: bit d of a record is (rec[d >> 3] >> (d & 7)) & 1."""
    bits = (np.asarray(bits) != 0).astype(np.uint8)
    count, n_bits = bits.shape
    out = np.zeros((count, (n_bits + 7) // 8), np.uint8)
    for d in range(n_bits):
        out[:, d >> 3] |= bits[:, d] << np.uint8(d & 7)
    return out


def unpack(records, n_bits):
    """records uint8[count, stride >= ceil(n_bits / 8)] -> uint8[count, n_bits]; bytes beyond and the high bits of the last byte are not looked at."""
    records = np.asarray(records, np.uint8)
    d = np.arange(n_bits)
    return (records[:, d >> 3] >> (d & 7).astype(np.uint8)) & np.uint8(1)


def default_layout(nsyn):
    """(n_bits, [bit_of_row per sector]): sector 0's rows, then sector 1's."""
    first = np.concatenate([[0], np.cumsum(nsyn)]).astype(np.int64)
    return int(first[-1]), [first[s] + np.arange(n, dtype=np.int64) for s, n in enumerate(nsyn)]


def gather(records, n_bits, tables):
    """The unpacker: per sector int8[count, nsyn], row r = bit tables[s][r] of the record, 0 where the table holds -1."""
    bits = unpack(records, n_bits)
    out = []
    for tab in tables:
        tab = np.asarray(tab, np.int64)
        assert ((tab >= -1) & (tab < n_bits)).all()
        out.append(np.where(tab[None, :] >= 0, bits[:, np.maximum(tab, 0)], 0).astype(np.int8))
    return out


def embed(syndromes, n_bits, tables, stride=None, fill=0, rng=None):
    """The inverse direction, for building test records: a record whose bit tables[s][r] is syndromes[s][:, r] (rows with -1 are dropped; a bit two rows
    name takes the later row).  Bits no row names are random when rng is given, else 0; every byte beyond ceil(n_bits / 8) and the unused high bits of the
    last byte are `fill` (0 or 1)."""
    count = syndromes[0].shape[0]
    bits = (rng.random((count, n_bits)) < 0.5).astype(np.uint8) if rng is not None else np.zeros((count, n_bits), np.uint8)
    for syn, tab in zip(syndromes, tables):
        tab = np.asarray(tab, np.int64)
        rows = np.flatnonzero(tab >= 0)
        bits[:, tab[rows]] = np.asarray(syn)[:, rows] & 1
    width = (n_bits + 7) // 8
    stride = width if stride is None else stride
    padded = np.full((count, 8 * stride), 1 if fill else 0, np.uint8)
    padded[:, :n_bits] = bits
    return pack(padded)


def predict(det, logmask):
    """uint64[count]: the XOR of the logical masks of the correction's ones (bit r = observable r)."""
    det, logmask = np.asarray(det), np.asarray(logmask, np.uint64)
    out = np.zeros(det.shape[0], np.uint64)
    for b in range(det.shape[0]):
        ones = np.flatnonzero(det[b] & 1)
        if ones.size:
            out[b] = np.bitwise_xor.reduce(logmask[ones])
    return out


def pred_bits(pred, k):
    """uint64[count] -> int8[count, k], column r = bit r"""
    pred = np.asarray(pred, np.uint64)
    return ((pred[:, None] >> np.arange(k, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int8) if k else np.zeros((pred.size, 0), np.int8)


def flags_of(conv, bad, zero):
    """the flags byte from per-sector lists of bool[count] (one or two sectors): bit s = conv, bit 2 + s = bad, bit 4 + s = zero syndrome"""
    out = np.zeros(np.asarray(conv[0]).shape[0], np.uint8)
    for s in range(len(conv)):
        out |= (np.asarray(conv[s]) != 0).astype(np.uint8) << np.uint8(s)
        out |= (np.asarray(bad[s]) != 0).astype(np.uint8) << np.uint8(2 + s)
        out |= (np.asarray(zero[s]) != 0).astype(np.uint8) << np.uint8(4 + s)
    return out
