"""Numpy restatement of the env record and of the snapshot image (include/hsrsim.h: hsr_snapshot_export; DESIGN.md "Snapshots"), written
from the documents, not from the library's source: the tests hold the two against each other.

record = the rows of   qpos nq | qvel nv | ctrl nu | mocap 3 | warm nv | time done bad nsteps tick 1 each | sepax 4 npair_sep |
                       septick npair_sep | trips 1 | xpos 3 nlink | xmat 9 nlink | lvel 6 nlink | ep_index ep_length ep_return 1 each
         with npair_sep = max(npair, 1); every row one 4-byte word per env
image  = header (56 bytes, little-endian) + uint32 [record words][capacity]
header = "HSRSNAP1" | u32 version = 1 | u32 header bytes = 56 | u64 fingerprint | i64 capacity | i32 nq nv nu nlink npair_sep | i32 record words
fingerprint = 64-bit FNV-1a of the model blob's bytes"""
import struct

import numpy as np

MAGIC, VERSION, HEADER = b"HSRSNAP1", 1, 56
HEADER_FMT = "<8sIIQq6i"
# byte offset of every header field (the tests corrupt them one by one)
OFFSETS = {"magic": 0, "version": 8, "header_bytes": 12, "fingerprint": 16, "capacity": 24, "nq": 32, "nv": 36, "nu": 40, "nlink": 44,
           "npair_sep": 48, "words": 52}


def fnv1a64(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for chunk in np.frombuffer(data, np.uint8).tolist():
        h = ((h ^ chunk) * 0x100000001b3) & 0xffffffffffffffff
    return h


def dims(m):
    return [m.nq, m.nv, m.nu, m.nlink, max(m.npair, 1)]


def fields(m):
    """(name, rows) in record order."""
    nq, nv, nu, nl, ns = dims(m)
    return [("qpos", nq), ("qvel", nv), ("ctrl", nu), ("mocap", 3), ("warm", nv), ("time", 1), ("done", 1), ("bad", 1), ("nsteps", 1), ("tick", 1),
            ("sepax", 4 * ns), ("septick", ns), ("trips", 1), ("xpos", 3 * nl), ("xmat", 9 * nl), ("lvel", 6 * nl), ("ep_index", 1),
            ("ep_length", 1), ("ep_return", 1)]


def record_words(m) -> int:
    return sum(rows for _, rows in fields(m))


def image(m, words_by_slot: np.ndarray) -> bytes:
    """words_by_slot uint32 [record words, capacity] -> image bytes."""
    w = np.ascontiguousarray(words_by_slot, "<u4")
    assert w.shape[0] == record_words(m)
    return struct.pack(HEADER_FMT, MAGIC, VERSION, HEADER, fnv1a64(m.to_bytes()), w.shape[1], *dims(m), w.shape[0]) + w.tobytes()


def parse(m, data: bytes):
    """image bytes -> {field: uint32 [rows, capacity]} (the header is checked against the model)."""
    magic, version, hb, fp, cap, *rest = struct.unpack(HEADER_FMT, data[:HEADER])
    assert (magic, version, hb, fp, rest) == (MAGIC, VERSION, HEADER, fnv1a64(m.to_bytes()), dims(m) + [record_words(m)])
    w = np.frombuffer(data, "<u4", offset=HEADER).reshape(record_words(m), cap)
    out, row = {}, 0
    for name, rows in fields(m):
        out[name] = w[row:row + rows]
        row += rows
    return out
