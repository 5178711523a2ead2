"""Table files ("ktab", DESIGN.md, Table files) on the CPU.  The numpy restatement the GPU tests compare against (tests/ktab_ref.py)
agrees with a pure-Python brute force over dicts and bytes and with the hand-worked files of tests/golden/ktab_known.json;
kt_table_file_info and kt_table_file_check (host only: no GPU) accept the restatement's files and reject every structural
corruption with a message that names it."""
import json
import pathlib
import struct
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import ktab_ref as R  # noqa: E402

from kmertools_amd import _lib, device  # noqa: E402


# ---- the restatement against a brute force --------------------------------------------------------------------------------

def brute_encode(k, table, s=None):
    """dict key -> count into a single-section file, byte by byte from the format text"""
    n = len(table)
    if s is None:
        cl = 0
        while (1 << cl) < max(n, 1):
            cl += 1
        t = min(24, max(0, cl - 3))
        s = (2 * k - t + 7) // 8
    p = max(0, 2 * k - 8 * s)
    items = sorted(table.items())
    out = bytearray(b"KTAB") + struct.pack("<III", 1, k, 0)
    overflow = [c for _, c in items if c >= 255]
    out += b"KSEC" + struct.pack("<IQQQ", s, n, len(overflow), sum(c for _, c in items))
    body = bytearray()
    for b in range((1 << p) + 1):  # offsets[b] = entries whose prefix is below b
        body += struct.pack("<Q", sum(1 for key, _ in items if (key >> (8 * s) if p else 0) < b))
    for key, _ in items:
        body += bytes((key >> (8 * j)) & 255 for j in range(s))
    body += bytes(min(c, 255) for _, c in items)
    for c in overflow:
        body += struct.pack("<I", c)
    body += b"\0" * (-len(body) % 8)
    return bytes(out + body)


def random_table(rng, k, n):
    keys = rng.choice(1 << (2 * k), size=n, replace=False) if 2 * k <= 20 else np.unique(rng.integers(0, 1 << (2 * k), n, dtype=np.uint64))
    pool = np.array([1, 2, 254, 255, 256, 65535, 65536, 0xFFFFFFFF], np.uint64)
    return {int(a): int(c) for a, c in zip(keys, rng.choice(pool, len(keys)))}


@pytest.mark.parametrize("k, n", [(1, 0), (1, 2), (3, 1), (4, 63), (5, 200), (8, 300), (12, 500), (16, 700), (31, 900)])
def test_restatement_equals_brute_force(k, n):
    rng = np.random.default_rng(1000 * k + n)
    table = random_table(rng, k, n)
    keys = np.array(list(table), np.uint64)
    counts = np.array([table[int(a)] for a in keys], np.uint32)
    data = R.encode(k, keys, counts)
    assert data == brute_encode(k, table)
    gk, sections = R.decode(data)
    assert gk == k and len(sections) == 1
    assert dict(zip(map(int, sections[0][0]), map(int, sections[0][1]))) == table
    n_ovf = sum(1 for c in table.values() if c >= 255)
    assert len(data) == R.FILE_HDR + R.section_size(k, len(table), n_ovf)
    for s in R.legal_s(k):  # every legal forced S decodes to the same table
        forced = R.encode(k, keys, counts, s)
        if R.prefix_bits(k, s) <= 8:  # (the brute force counts the entries below every bucket)
            assert forced == brute_encode(k, table, s)
        assert dict(zip(*map(lambda a: map(int, a), R.decode(forced)[1][0]))) == table
        assert len(forced) == R.FILE_HDR + R.section_size(k, len(table), n_ovf, s)


def test_bytes_do_not_depend_on_order():
    rng = np.random.default_rng(7)
    keys = rng.choice(1 << 20, 400, replace=False).astype(np.uint64)
    counts = rng.integers(1, 600, 400).astype(np.uint32)
    perm = rng.permutation(400)
    assert R.encode(10, keys, counts) == R.encode(10, keys[perm], counts[perm])


def test_writer_S():
    assert (R.pick_s(31, 363_000_000), R.prefix_bits(31, 5)) == (5, 22)  # 6 bytes an entry and 32 MB of offsets
    assert R.pick_s(31, 0) == R.pick_s(31, 1) == R.pick_s(31, 8) == 8
    assert R.pick_s(31, 1 << 40) == 5  # t stops at 24
    assert [R.pick_s(1, n) for n in (0, 1, 2, 4)] == [1, 1, 1, 1]
    for k in range(1, 32):
        for n in (0, 1, 8, 9, 64, 65, 1 << 12, 1 << 20, 1 << 30):
            if n <= 1 << (2 * k):
                assert R.prefix_bits(k, R.pick_s(k, n)) <= min(24, max(0, R.ceil_log2(max(n, 1)) - 3))


def test_known_answers():
    known = json.loads((ROOT / "tests" / "golden" / "ktab_known.json").read_text())
    assert len(known["cases"]) >= 3
    for c in known["cases"]:
        want = bytes.fromhex(c["hex"].replace(" ", ""))
        assert R.encode(c["k"], c["keys"], c["counts"], c["s"]) == want, c["name"]
        k, sections = R.decode(want)
        assert k == c["k"] and list(map(int, sections[0][0])) == c["keys"] and list(map(int, sections[0][1])) == c["counts"]


# ---- the host ABI -------------------------------------------------------------------------------------------------------------

K = 9  # B = 18: S = 1 gives P = 10, the writer's S for a few hundred entries is 2 (P = 2)


def sample(seed=3, n=300, k=K):
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(1 << (2 * k), n, replace=False).astype(np.uint64))
    counts = rng.choice(np.array([1, 7, 254, 255, 300, 70000], np.uint32), n)
    return keys, counts


def test_abi_declared_and_bound():
    header = (ROOT / "include" / "kmertools_hip.h").read_text()
    for name in ("kt_table_file_info", "kt_table_file_check", "kt_ctr_save", "kt_ctr_add_file"):
        assert "int %s(" % name in header and name in _lib.SYMBOLS
    assert "#define KT_ERR_IO 7" in header and _lib.KT_ERR_IO == 7


def test_info_and_check_accept_good_files(tmp_path):
    keys, counts = sample()
    total = int(counts.astype(np.uint64).sum())
    for s in [None] + R.legal_s(K):
        path = tmp_path / ("s%s.ktab" % s)
        R.write_file(path, K, [(keys, counts)], s)
        assert device.table_file_info(path) == {"k": K, "sections": 1, "entries": 300, "occurrences": total}
        device.table_file_check(path)
    path = tmp_path / "three.ktab"
    R.write_file(path, K, [(keys, counts), (keys[:0], counts[:0]), (keys[::2], counts[::2])])
    assert device.table_file_info(path) == {"k": K, "sections": 3, "entries": 450,
                                            "occurrences": total + int(counts[::2].astype(np.uint64).sum())}
    device.table_file_check(path)
    path = tmp_path / "p24.ktab"  # k = 13: S = 1 leaves P = 18; k = 16, S = 1 would leave 24
    R.write_file(path, 16, [(keys, counts)], 1)
    assert device.table_file_info(path)["k"] == 16
    device.table_file_check(path)


def rejected(call, path, *words):
    with pytest.raises(_lib.KmertoolsError) as e:
        call(path)
    assert e.value.code == _lib.KT_ERR_IO, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def both_reject(path, *words):
    rejected(device.table_file_info, path, *words)
    rejected(device.table_file_check, path, *words)


def test_null_and_missing(tmp_path):
    L = _lib.lib()
    assert L.kt_table_file_check(None) == _lib.KT_ERR_ARG
    assert L.kt_table_file_info(None, None, None, None, None) == _lib.KT_ERR_ARG
    both_reject(tmp_path / "nothing.ktab", "cannot open")
    both_reject(tmp_path, "not a regular file")


def test_header_corruptions(tmp_path):
    keys, counts = sample()
    good = R.encode(K, keys, counts)
    path = tmp_path / "t.ktab"
    path.write_bytes(b"KTAX" + good[4:])
    both_reject(path, "bad magic")
    path.write_bytes(good[:4] + struct.pack("<I", 2) + good[8:])
    both_reject(path, "version 2")
    path.write_bytes(good[:8] + struct.pack("<I", 32) + good[12:])
    both_reject(path, "bad file header")
    path.write_bytes(good[:R.FILE_HDR] + b"KSEX" + good[R.FILE_HDR + 4:])
    both_reject(path, "section 0", "bad section magic")


def test_truncations(tmp_path):
    keys, counts = sample(n=301)  # (odd: the section ends with padding)
    parts = [R.file_header(K)] + R.section_parts(K, keys, counts)
    good = b"".join(parts)
    assert all(len(p) for p in parts)  # header, offsets, suffix, count bytes, overflow, padding: all there
    path = tmp_path / "t.ktab"
    ends = np.cumsum([len(p) for p in parts])
    for cut in sorted({0, 1, R.FILE_HDR - 1} | {int(e) for e in ends[:-1]} | {int(e) - 1 for e in ends}):
        path.write_bytes(good[:cut])
        both_reject(path, "truncated")
    # ... and behind a whole section: the second one cut at each of its part boundaries and one byte short of its end
    sec = b"".join(parts[1:])
    ends2 = np.cumsum([len(p) for p in parts[1:]])
    for cut in sorted({int(e) for e in ends2[:-1]} | {len(sec) - 1}):
        path.write_bytes(good + sec[:cut])
        both_reject(path, "section 1", "truncated")
    path.write_bytes(good + sec)
    device.table_file_check(path)


def test_trailing_bytes(tmp_path):
    keys, counts = sample()
    good = R.encode(K, keys, counts)
    path = tmp_path / "t.ktab"
    for extra in (b"\0", b"\0" * 8, b"\0" * 31, b"\0" * 32, b"x" * 100):
        path.write_bytes(good + extra)
        both_reject(path, "trailing bytes")


def with_header(data, s=None, n=None, n_overflow=None):
    h = R.FILE_HDR
    S, N, V, O = struct.unpack_from("<IQQQ", data, h + 4)
    return data[:h + 4] + struct.pack("<IQQQ", S if s is None else s, N if n is None else n, V if n_overflow is None else n_overflow,
                                      O) + data[h + R.SEC_HDR:]


def test_section_header_corruptions(tmp_path):
    keys, counts = sample()
    path = tmp_path / "t.ktab"
    good = R.encode(K, keys, counts)
    for s in (0, 9, 0xFFFFFFFF):
        path.write_bytes(with_header(good, s=s))
        both_reject(path, "illegal S")
    path.write_bytes(with_header(good, n_overflow=301))
    both_reject(path, "n_overflow > n")
    path.write_bytes(with_header(good, n=1 << 62))
    both_reject(path, "truncated")
    big = R.encode(31, keys, counts)  # B = 62: S = 4 would leave P = 30
    path.write_bytes(with_header(big, s=4))
    both_reject(path, "P > 24")
    path.write_bytes(with_header(R.encode(17, keys, counts, 2), s=1))  # B = 34: S = 1 leaves 26
    both_reject(path, "P > 24")


def test_offsets_corruptions(tmp_path):
    keys, counts = sample()
    path = tmp_path / "t.ktab"
    good = R.encode(K, keys, counts, 1)  # P = 10: 1025 offsets
    at = R.FILE_HDR + R.SEC_HDR
    offsets = np.frombuffer(good, "<u8", 1025, at).copy()
    assert offsets[0] == 0 and offsets[-1] == 300 and 0 < offsets[500] < 300

    def write(o):
        path.write_bytes(good[:at] + o.astype("<u8").tobytes() + good[at + 8 * 1025:])
        assert device.table_file_info(path)["entries"] == 300  # the header chain is whole: info does not read offsets[]
        return path

    o = offsets.copy()
    o[500] = o[499] - 1 if o[499] else o[501] + 1
    if o[499] == 0:
        o[501] = o[500] - 1
    rejected(device.table_file_check, write(o), "offsets decrease")
    o = offsets.copy()
    o[0] = 1
    rejected(device.table_file_check, write(o), "offsets[0] is not 0")
    o = offsets.copy()
    o[o == 300] = 299
    rejected(device.table_file_check, write(o), "the last offset is not n")
    o = offsets.copy()
    o[-1] = 301
    rejected(device.table_file_check, write(o), "an offset > n")
    o = offsets.copy()
    o[700] = 1 << 63
    rejected(device.table_file_check, write(o), "an offset > n")
    device.table_file_check(write(offsets))
