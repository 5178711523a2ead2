"""The restatement of the HyperLogLog calls (no test in here): the registers of a batch from the oracle's k-mers with numpy,
Ertl's improved raw estimator in Python floats, evaluated in the order include/kmertools_hip.h prints, the inverse of the
hash's finaliser (for inputs whose hashes are chosen), and a pure-Python integer brute force of the registers that shares
nothing with either."""
import math

import numpy as np

U = np.uint64
MASK = (1 << 64) - 1
MIN_P, MAX_P = 4, 16


def mix64(z):
    """ktd::mix64 (splitmix64's finaliser) over a u64 array, as in test_sketch.py"""
    z = np.asarray(z, np.uint64) + U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def mix64_int(z):
    """the same on one Python integer"""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


_INV1 = pow(0xBF58476D1CE4E5B9, -1, 1 << 64)
_INV2 = pow(0x94D049BB133111EB, -1, 1 << 64)


def _unshift(x, s):
    """y with y ^ (y >> s) == x"""
    y, t = x, x >> s
    while t:
        y ^= t
        t >>= s
    return y


def unmix64(h):
    """the z with mix64_int(z) == h (the finaliser is a bijection of the 64-bit words)"""
    z = _unshift(h, 31)
    z = (z * _INV2) & MASK
    z = _unshift(z, 27)
    z = (z * _INV1) & MASK
    z = _unshift(z, 30)
    return (z - 0x9E3779B97F4A7C15) & MASK


def ranks_of(h, p):
    """(register index, rank) of every hash of a u64 array: j = h >> q, r = 1 + leading zeros of the low q bits as a q-bit
    word (q + 1 when they are all zero)"""
    q = 64 - p
    h = np.asarray(h, np.uint64)
    j = (h >> U(q)).astype(np.int64)
    low = h & U((1 << q) - 1)
    # bit length of low: by halving (no float: q can be 60)
    bl = np.zeros(len(h), np.int64)
    rest = low.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = rest >= U(1 << s)
        bl[big] += s
        rest[big] >>= U(s)
    bl += (rest > 0)
    return j, (q - bl + 1).astype(np.int64)


def registers_of_hashes(h, p, into=None):
    reg = np.zeros(1 << p, np.uint8) if into is None else into
    if len(h):
        j, r = ranks_of(h, p)
        np.maximum.at(reg, j, r.astype(np.uint8))
    return reg


def canonical_kmers(oracle, bases, offsets, k):
    """the canonical k-mers of every read of a CSR batch, with multiplicity, one u64 array"""
    out = []
    o = np.asarray(offsets).astype(np.int64)
    for i in range(len(o) - 1):
        if o[i + 1] - o[i] < k:
            continue
        f, r, _ = oracle.kmers(np.ascontiguousarray(bases[o[i]:o[i + 1]]).tobytes(), k)
        out.append(np.minimum(f, r))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def registers(oracle, bases, offsets, k, p, seed=0, into=None):
    """-> (registers u8[2^p], windows with multiplicity): what kt_card_add_reads leaves of a batch (combined into `into`)"""
    km = canonical_kmers(oracle, bases, offsets, k)
    return registers_of_hashes(mix64(km ^ U(seed)), p, into), len(km)


def brute_registers(kmers, p, seed=0):
    """the same from Python integers, one k-mer at a time, the rank by shifting"""
    q = 64 - p
    reg = [0] * (1 << p)
    for x in kmers:
        h = mix64_int(int(x) ^ seed)
        j, low, r = h >> q, h & ((1 << q) - 1), 1
        while r <= q and not (low >> (q - r)) & 1:
            r += 1
        reg[j] = max(reg[j], r)
    return np.array(reg, np.uint8)


def sigma(x):
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        zp = z
        z += x * y
        y += y
        if zp == z:
            return z


def tau(x):
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        zp = z
        y *= 0.5
        z -= (1.0 - x) ** 2 * y
        if zp == z:
            return z / 3.0


def estimate(reg):
    """-> (estimate, zero registers); ValueError for a register above q + 1 (the library's KT_ERR_ARG)"""
    m = len(reg)
    p = m.bit_length() - 1
    assert m == 1 << p and MIN_P <= p <= MAX_P
    q = 64 - p
    c = np.bincount(np.asarray(reg, np.int64), minlength=q + 2)
    if len(c) > q + 2:
        raise ValueError("a register above q + 1")
    z = m * tau(1.0 - float(c[q + 1]) / m)
    for v in range(q, 0, -1):
        z = 0.5 * (z + float(c[v]))
    z += m * sigma(float(c[0]) / m)
    num = m * m / (2.0 * math.log(2.0))
    return (num / z if z != 0.0 else math.inf), int(c[0])


def rel_error(p):
    return 1.04 / math.sqrt(float(1 << p))


def slots_for_estimate(est, p):
    """what --estimate-size asks for E distinct k-mers: 1.9 slots for the estimate and five standard errors, at least 1024"""
    e = int(math.ceil(est * (1.0 + 5.0 * rel_error(p))))
    return max(1024, e + e // 10 * 9)


def bound_slots(n_bases_bound, k):
    """the plan without the flag: the input's bases as its distinct k-mers, at most the canonical k-mers of k <= 15"""
    d = n_bases_bound
    if k <= 15:
        n4k = 1 << (2 * k)
        d = min(d, n4k // 2 if k & 1 else (n4k + (1 << k)) // 2)
    return max(1024, d + d // 10 * 9)
