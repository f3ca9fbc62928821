"""Big-integer reference of b2f_ntt_columns_dev (Python ints): the definitions of include/b2f.h
as O(n^2) sums, an iterative radix-2 NTT with the forward / inverse wrappers, and the limb
packing of the four B2F_FP_* forms."""
import numpy as np

P_PALLAS = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
P_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
R256 = 1 << 256


def modulus(form):
    return P_BN254 if form & 2 else P_PALLAS


def ntt(x, w, p):
    """out[i] = sum_j x[j] w^(i j) mod p, len(x) = 2^k, w a primitive 2^k-th root of unity."""
    n = len(x)
    k = n.bit_length() - 1
    assert 1 << k == n
    a = [0] * n
    for i, v in enumerate(x):
        a[int(format(i, "0%db" % k)[::-1], 2) if k else 0] = v
    half = 1
    while half < n:
        wl = pow(w, n // (2 * half), p)
        tw = [1] * half
        for t in range(1, half):
            tw[t] = tw[t - 1] * wl % p
        for base in range(0, n, 2 * half):
            for t in range(half):
                u = a[base + t]
                v = a[base + t + half] * tw[t] % p
                a[base + t] = (u + v) % p
                a[base + t + half] = (u - v) % p
        half *= 2
    return a


def forward(x, k, w, shift, p):
    """out[i] = sum_j x[j] (shift w^i)^j; x shorter than 2^k is zero-padded."""
    n = 1 << k
    s, y = 1, []
    for v in list(x) + [0] * (n - len(x)):
        y.append(v * s % p)
        s = s * shift % p
    return ntt(y, w, p)


def inverse(x, k, w, shift, p):
    """out[j] = shift^-j n^-1 sum_i x[i] w^(-i j)"""
    n = 1 << k
    assert len(x) == n
    y = ntt(list(x), pow(w, p - 2, p), p)
    si, c, out = pow(shift, p - 2, p), pow(n, p - 2, p), []
    for v in y:
        out.append(v * c % p)
        c = c * si % p
    return out


def forward_def(x, k, w, shift, p):
    n = 1 << k
    return [sum(v * pow(shift * pow(w, i, p), j, p) for j, v in enumerate(x)) % p for i in range(n)]


def inverse_def(x, k, w, shift, p):
    n = 1 << k
    ninv, si, wi = pow(n, p - 2, p), pow(shift, p - 2, p), pow(w, p - 2, p)
    return [pow(si, j, p) * ninv * sum(v * pow(wi, i * j, p) for i, v in enumerate(x)) % p
            for j in range(n)]


def horner(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def pack(vals, form):
    """Field elements (ints < p) as uint64 [len, 4] limbs in `form`."""
    p = modulus(form)
    if form & 1:
        vals = [v * R256 % p for v in vals]
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals),
                         dtype=np.uint64).reshape(-1, 4).copy()


def unpack(limbs, form):
    """uint64 [len, 4] limbs in `form` -> ints (canonical values)."""
    p = modulus(form)
    raw = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    vals = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    if form & 1:
        rinv = pow(R256, p - 2, p)
        vals = [v * rinv % p for v in vals]
    return vals


def random_elements(rng, count, p):
    raw = rng.bytes(40 * count)
    return [int.from_bytes(raw[40 * i:40 * i + 40], "little") % p for i in range(count)]
