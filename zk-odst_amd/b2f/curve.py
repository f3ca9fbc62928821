"""Host-side constants of the two commitment curves and the point layout of b2f_msm_dev.

Vesta (forms 0/1: y^2 = x^3 + 5 over pasta Fq, group order pasta Fp) and BN254 G1 (forms 2/3:
y^2 = x^3 + 3 over bn256::Fq, group order bn256::Fr): the curve a column in `form` is committed
on is the one whose scalar field the form names.

A point on the device is affine, (x, y), each coordinate four little-endian u64 limbs in
base-field Montgomery form (x R mod q, R = 2^256): 8 limbs, 64 bytes; the identity is all zeros.
pack_points / unpack_points convert between that and pairs of Python ints (None: the identity).
"""
import numpy as np

from . import _lib, field

VESTA, BN254_G1 = 0, 1
# the base field's modulus q, the constant b, the group order r (the scalar field's modulus) and
# a generator
BASE_MODULUS = {VESTA: 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001,
                BN254_G1: 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47}
B = {VESTA: 5, BN254_G1: 3}
ORDER = {VESTA: field.MODULUS[field.PALLAS], BN254_G1: field.MODULUS[field.BN254]}
GENERATOR = {VESTA: (BASE_MODULUS[VESTA] - 1, 2), BN254_G1: (1, 2)}
R = 1 << 256


def of_form(form):
    """The curve a B2F_FP_* form's columns are committed on."""
    return BN254_G1 if int(form) & 2 else VESTA


def on_curve(curve, pt):
    if pt is None:
        return True
    q = BASE_MODULUS[curve]
    x, y = pt
    return 0 <= x < q and 0 <= y < q and (y * y - x * x * x - B[curve]) % q == 0


def pack_points(curve, pts):
    """[(x, y) | None] -> uint64 [n, 8] Montgomery limbs (None: the identity, all zeros)."""
    q = BASE_MODULUS[curve]
    raw = bytearray()
    for pt in pts:
        if pt is None:
            raw += bytes(64)
            continue
        x, y = pt
        if not (0 <= x < q and 0 <= y < q):
            raise _lib.B2FError(_lib.ERR_ARG, "a coordinate is not a reduced base-field element")
        raw += (x * R % q).to_bytes(32, "little") + (y * R % q).to_bytes(32, "little")
    return np.frombuffer(bytes(raw), dtype=np.uint64).reshape(-1, 8).copy()


def unpack_points(curve, limbs):
    """uint64 (or int64) [n, 8] Montgomery limbs -> [(x, y) | None]."""
    q = BASE_MODULUS[curve]
    rinv = pow(R, -1, q)
    raw = np.ascontiguousarray(limbs).view(np.uint64).reshape(-1, 8).tobytes()
    out = []
    for i in range(0, len(raw), 64):
        x = int.from_bytes(raw[i:i + 32], "little")
        y = int.from_bytes(raw[i + 32:i + 64], "little")
        out.append(None if x == 0 and y == 0 else (x * rinv % q, y * rinv % q))
    return out
