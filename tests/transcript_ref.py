"""Pure-Python restatement of the device transcript (csrc/b2f_transcript.h) and of the host side of
the one-call opening (b2f_ipa_open_dev), on tests/msm_ref.py and tests/ipa_ref.py.

`Blake2b` keeps (h, t, buffer, count) explicitly -- the words of the device state -- so a test can
compare the state word for word after every step: BLAKE2b with a 64-byte digest, no key, the
personalisation "Halo2-Transcript", a full buffer compressed only when the next byte arrives (the
lazy last block), buffer bytes at and past the count kept zero. tests/test_transcript_ref.py pins it
to hashlib.

`Transcript` is halo2's Blake2bWrite / Challenge255 (halo2_proofs 0.3.0 transcript.rs) on top:
common_point absorbs the byte 1 and the two canonical coordinates (32 little-endian bytes each),
common_scalar the byte 2 and the canonical scalar, squeeze absorbs the byte 0, finalises a copy and
reduces the 64 digest bytes, read little-endian, modulo the scalar field's r. The identity (None)
absorbs the byte 1 and 64 zero bytes, which is the device's definition (halo2 refuses it).

`opening_points` / `opening_known` run create_proof's loop with the transcript in it: generators as
affine points, or as known multiples of the curve's generator (every point one gen_mul)."""
import ipa_ref as ir
import msm_ref as mr

IV = (0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
      0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179)
SIGMA = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15),
         (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3),
         (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4),
         (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8),
         (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13),
         (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
         (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11),
         (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10),
         (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5),
         (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))
M64 = (1 << 64) - 1
PERSON = b"Halo2-Transcript"
STATE_WORDS = 32


def _rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


def compress(h, block, t, last):
    """One BLAKE2b compression (RFC 7693): h' of h, a 128-byte block, the byte counter and the flag."""
    m = [int.from_bytes(block[8 * i:8 * i + 8], "little") for i in range(16)]
    v = list(h) + list(IV)
    v[12] ^= t & M64
    v[13] ^= t >> 64
    if last:
        v[14] ^= M64

    def g(a, b, c, d, x, y):
        v[a] = (v[a] + v[b] + x) & M64
        v[d] = _rotr(v[d] ^ v[a], 32)
        v[c] = (v[c] + v[d]) & M64
        v[b] = _rotr(v[b] ^ v[c], 24)
        v[a] = (v[a] + v[b] + y) & M64
        v[d] = _rotr(v[d] ^ v[a], 16)
        v[c] = (v[c] + v[d]) & M64
        v[b] = _rotr(v[b] ^ v[c], 63)

    for r in range(12):
        s = SIGMA[r % 10]
        g(0, 4, 8, 12, m[s[0]], m[s[1]])
        g(1, 5, 9, 13, m[s[2]], m[s[3]])
        g(2, 6, 10, 14, m[s[4]], m[s[5]])
        g(3, 7, 11, 15, m[s[6]], m[s[7]])
        g(0, 5, 10, 15, m[s[8]], m[s[9]])
        g(1, 6, 11, 12, m[s[10]], m[s[11]])
        g(2, 7, 8, 13, m[s[12]], m[s[13]])
        g(3, 4, 9, 14, m[s[14]], m[s[15]])
    return [h[i] ^ v[i] ^ v[8 + i] for i in range(8)]


class Blake2b:
    """BLAKE2b-512, no key, personalised; the state explicit."""

    def __init__(self, person=PERSON):
        person = person.ljust(16, b"\0")
        self.h = list(IV)
        self.h[0] ^= 0x01010040  # digest 64, key 0, fanout 1, depth 1
        self.h[6] ^= int.from_bytes(person[:8], "little")
        self.h[7] ^= int.from_bytes(person[8:], "little")
        self.t = 0  # bytes compressed so far
        self.buf = bytearray(128)
        self.count = 0

    def copy(self):
        c = Blake2b.__new__(Blake2b)
        c.h, c.t, c.buf, c.count = list(self.h), self.t, bytearray(self.buf), self.count
        return c

    def update(self, data):
        for byte in data:
            if self.count == 128:  # the block is not the last one after all
                self.t += 128
                self.h = compress(self.h, self.buf, self.t, False)
                self.buf = bytearray(128)
                self.count = 0
            self.buf[self.count] = byte
            self.count += 1
        return self

    def digest(self):
        """The 64-byte digest of the bytes so far; the state goes on."""
        h = compress(self.h, self.buf, self.t + self.count, True)
        return b"".join(x.to_bytes(8, "little") for x in h)

    def words(self):
        """The 32 u64 words of the device state (include/b2f.h)."""
        w = list(self.h) + [self.t & M64, self.t >> 64]
        w += [int.from_bytes(self.buf[8 * i:8 * i + 8], "little") for i in range(16)]
        return w + [self.count] + [0] * 5


def point_bytes(pt):
    if pt is None:
        return b"\1" + bytes(64)
    return b"\1" + pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")


def scalar_bytes(s):
    return b"\2" + int(s).to_bytes(32, "little")


class Transcript:
    """Blake2bWrite / Challenge255 for the curve cv (0 Vesta, 1 BN254 G1)."""

    def __init__(self, cv, hasher=None):
        self.cv = cv
        self.hash = hasher if hasher is not None else Blake2b()

    def copy(self):
        return Transcript(self.cv, self.hash.copy())

    def common_point(self, pt):
        self.hash.update(point_bytes(pt))

    def common_scalar(self, s):
        self.hash.update(scalar_bytes(s))

    def squeeze(self):
        self.hash.update(b"\0")
        return int.from_bytes(self.hash.digest(), "little") % mr.ORDER[self.cv]

    def words(self):
        return self.hash.words()


def _rounds(cv, p, b, z, rand, tr, f, cross, fold, blind):
    """create_proof's loop. cross(p, G) -> the raw (L, R); blind(raw, scalar on U, scalar on W) ->
    the blinded term as a point; fold(G, u) -> the folded generators. Returns
    dict(lr = [(L_j, R_j)], u = [u_j], c, f, p, b, g)."""
    r = mr.ORDER[cv]
    p, b = list(p), list(b)
    lrs, us = [], []
    j = 0
    while len(p) > 1:
        raw_l, raw_r = cross(p)
        vl, vr = ir.values(cv, p, b)
        l_rand, r_rand = rand[2 * j], rand[2 * j + 1]
        L = blind(raw_l, vl * z % r, l_rand)
        R = blind(raw_r, vr * z % r, r_rand)
        tr.common_point(L)
        tr.common_point(R)
        u = tr.squeeze()
        ui = pow(u, -1, r)
        f = (f + l_rand * ui + r_rand * u) % r
        p, b = ir.fold_scalars(cv, p, b, u)
        fold(u)
        lrs.append((L, R))
        us.append(u)
        j += 1
    c = p[0]
    tr.common_scalar(c)
    tr.common_scalar(f)
    return dict(lr=lrs, u=us, c=c, f=f, p=p, b=b)


def opening_points(cv, p, b, G, U, W, z, rand, tr, f):
    """The opening by plain point arithmetic: G, U, W affine points. The result's g is the folded G."""
    state = {"G": list(G)}

    def cross(p_):
        return ir.round_points(cv, p_, state["G"])

    def blind(raw, su, sw):
        return mr.add(cv, mr.add(cv, raw, mr.mul(cv, su, U)), mr.mul(cv, sw, W))

    def fold(u):
        state["G"] = ir.fold_points(cv, state["G"], u)

    out = _rounds(cv, p, b, z, rand, tr, f, cross, fold, blind)
    out["g"] = state["G"]
    return out


def opening_known(cv, p, b, gm, um, wm, z, rand, tr, f):
    """The same on known multiples of the curve's generator: G_i = gm[i] Gen, U = um Gen, W = wm Gen.
    Every point is one gen_mul; the result's lr are affine points, its g the folded multiples."""
    r = mr.ORDER[cv]
    state = {"gm": list(gm)}

    def cross(p_):
        return ir.round_known(cv, p_, state["gm"])

    def blind(raw, su, sw):
        return mr.gen_mul(cv, (raw + su * um + sw * wm) % r)

    def fold(u):
        state["gm"] = ir.fold_known(cv, state["gm"], u)

    out = _rounds(cv, p, b, z, rand, tr, f, cross, fold, blind)
    out["g"] = state["gm"]
    return out
