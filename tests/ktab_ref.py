"""The "ktab" table file format (DESIGN.md, Table files) restated in numpy: encode and decode, independent of the library.

A file is a 16-byte header and one or more sections; encode_section() makes one section from (keys, counts), with the
writer's S or a forced one, write_file() strings sections together, decode() reads everything back.  Nothing here is fast.
"""
import struct

import numpy as np

FILE_MAGIC, SEC_MAGIC, VERSION = b"KTAB", b"KSEC", 1
FILE_HDR, SEC_HDR, MAX_P = 16, 32, 24


def ceil_log2(x):
    return 0 if x <= 1 else int(x - 1).bit_length()


def pick_s(k, n):
    """the writer's suffix bytes: t = min(24, max(0, ceil_log2(max(n, 1)) - 3)), S = ceil((2k - t) / 8)"""
    t = min(MAX_P, max(0, ceil_log2(max(n, 1)) - 3))
    return max(1, -(-(2 * k - t) // 8))


def prefix_bits(k, s):
    return max(0, 2 * k - 8 * s)


def legal_s(k):
    return [s for s in range(1, 9) if prefix_bits(k, s) <= MAX_P]


def file_header(k):
    return FILE_MAGIC + struct.pack("<III", VERSION, k, 0)


def section_parts(k, keys, counts, s=None, sort=True):
    """the parts of one section, in file order: header, offsets, suffix bytes, count bytes, overflow, padding"""
    keys = np.asarray(keys, np.uint64)
    counts = np.asarray(counts, np.uint32)
    if sort:
        order = np.argsort(keys, kind="stable")
        keys, counts = keys[order], counts[order]
    n = len(keys)
    s = pick_s(k, n) if s is None else s
    p = prefix_bits(k, s)
    prefix = (keys >> np.uint64(8 * s)) if p else np.zeros(n, np.uint64)
    offsets = np.searchsorted(prefix, np.arange((1 << p) + 1, dtype=np.uint64), side="left").astype("<u8")
    offsets[-1] = n
    suffix = np.zeros((n, s), np.uint8)
    for b in range(s):
        suffix[:, b] = ((keys >> np.uint64(8 * b)) & np.uint64(255)).astype(np.uint8)
    cbytes = np.minimum(counts, 255).astype(np.uint8)
    overflow = counts[counts >= 255].astype("<u4")
    header = SEC_MAGIC + struct.pack("<IQQQ", s, n, len(overflow), int(counts.astype(np.uint64).sum()))
    body = [offsets.tobytes(), suffix.tobytes(), cbytes.tobytes(), overflow.tobytes()]
    body.append(b"\0" * (-sum(map(len, body)) % 8))
    return [header] + body


def encode_section(k, keys, counts, s=None, sort=True):
    return b"".join(section_parts(k, keys, counts, s, sort))


def encode(k, keys, counts, s=None):
    """a whole single-section file"""
    return file_header(k) + encode_section(k, keys, counts, s)


def write_file(path, k, sections, s=None):
    """sections: a list of (keys, counts)"""
    with open(path, "wb") as f:
        f.write(file_header(k))
        for keys, counts in sections:
            f.write(encode_section(k, keys, counts, s))


def section_size(k, n, n_overflow, s=None):
    """header + (S + 1) n + 8 (2^P + 1) + 4 n_overflow, padded to 8"""
    s = pick_s(k, n) if s is None else s
    raw = (s + 1) * n + 8 * ((1 << prefix_bits(k, s)) + 1) + 4 * n_overflow
    return SEC_HDR + raw + (-raw) % 8


def decode(data):
    """(k, [(keys, counts), ...]) of a file's bytes; asserts what the format promises"""
    assert data[:4] == FILE_MAGIC
    version, k, zero = struct.unpack_from("<III", data, 4)
    assert version == VERSION and zero == 0
    pos, sections = FILE_HDR, []
    while pos < len(data):
        assert data[pos:pos + 4] == SEC_MAGIC
        s, n, n_ovf, occ = struct.unpack_from("<IQQQ", data, pos + 4)
        pos += SEC_HDR
        p = prefix_bits(k, s)
        assert 1 <= s <= 8 and p <= MAX_P and n_ovf <= n
        nb1 = (1 << p) + 1
        start = pos
        offsets = np.frombuffer(data, "<u8", nb1, pos)
        pos += 8 * nb1
        suffix = np.frombuffer(data, np.uint8, n * s, pos).reshape(n, s)
        pos += n * s
        cbytes = np.frombuffer(data, np.uint8, n, pos)
        pos += n
        overflow = np.frombuffer(data, "<u4", n_ovf, pos)
        pos += 4 * n_ovf
        pos += -(pos - start) % 8
        assert offsets[0] == 0 and offsets[-1] == n and np.all(np.diff(offsets.astype(np.int64)) >= 0)
        keys = np.repeat(np.arange(nb1 - 1, dtype=np.uint64), np.diff(offsets).astype(np.int64)) << np.uint64(8 * s if p else 0)
        for b in range(s):
            keys = keys | (suffix[:, b].astype(np.uint64) << np.uint64(8 * b))
        counts = cbytes.astype(np.uint32)
        esc = cbytes == 255
        assert int(esc.sum()) == n_ovf and not np.any(cbytes == 0)
        counts[esc] = overflow
        assert int(counts.astype(np.uint64).sum()) == occ
        assert np.all(keys[1:] > keys[:-1])
        sections.append((keys, counts))
    assert pos == len(data)
    return k, sections
