"""Big-integer reference of b2f_group_ntt_dev on tests/msm_ref.py (the curves) and tests/ntt_ref.py
(the field transform), two ways:

  (a) by definition, in plain point arithmetic: out[i] = [c] sum_j [w^(+-i j)] in[j] with msm_ref's
      mul and add, O(n^2) scalar multiplications: small k only;
  (b) the known-multiples shortcut: for in[j] = b_j G the transform is linear in the multiples,
      out[i] = [NTT_r(b)[i]] G, a field NTT modulo the group order followed by one fixed-base
      multiplication per output.

Curves are msm_ref's: 0 Vesta, 1 BN254 G1; a form's curve is msm_ref.curve_of_form(form). Points are
affine (x, y) tuples, the identity None. The domain's generator is derived here from the scalar
field's own constants (nothing imported from the package)."""
import msm_ref as mr
import ntt_ref as nr

# multiplicative generator and 2-adicity of the two group orders (pasta Fp, bn256::Fr)
GENERATOR = (5, 7)
TWO_ADICITY = (32, 28)


def omega(cv, k):
    """The generator of the 2^k domain of curve cv's scalar field: ROOT_OF_UNITY squared S - k times."""
    r, s = mr.ORDER[cv], TWO_ADICITY[cv]
    assert 0 <= k <= s
    root = pow(GENERATOR[cv], (r - 1) >> s, r)
    return pow(root, 1 << (s - k), r)


def transform_def(cv, pts, k, inverse=False):
    """(a): the definition. forward out[i] = sum_j [w^(i j)] in[j]; inverse out[i] = [n^-1] sum_j
    [w^(-i j)] in[j]."""
    n, r = 1 << k, mr.ORDER[cv]
    assert len(pts) == n
    w = omega(cv, k)
    if inverse:
        w = pow(w, r - 2, r)
    c = pow(n, r - 2, r) if inverse else 1
    out = []
    for i in range(n):
        acc = None
        for j, pt in enumerate(pts):
            acc = mr.add(cv, acc, mr.mul(cv, pow(w, i * j, r), pt))
        out.append(mr.mul(cv, c, acc))
    return out


def multiples(cv, b, k, inverse=False):
    """The multiples of G of the transform of (b_j G): the field NTT of b modulo the group order."""
    r = mr.ORDER[cv]
    w = omega(cv, k)
    return nr.inverse(list(b), k, w, 1, r) if inverse else nr.forward(list(b), k, w, 1, r)


def gen_mul_many(cv, ms):
    """[m G for m in ms] from msm_ref's fixed-base table with one inversion for all of them (a zero
    multiple is the identity, None): what keeps a 2^12-point expectation to about a second."""
    t = mr._table(cv)
    js = []
    for m in ms:
        acc = (1, 1, 0)
        for j in range(32):
            d = (m >> (8 * j)) & 255
            if d:
                acc = mr.jac_add(cv, acc, t[j][d])
        js.append(acc)
    live = [i for i, p in enumerate(js) if p[2] != 0]
    out = [None] * len(js)
    for i, pt in zip(live, mr.batch_affine(cv, [js[i] for i in live])):
        out[i] = pt
    return out


def transform_known(cv, b, k, inverse=False):
    """(b): the transform of the points b_j G as points."""
    return gen_mul_many(cv, multiples(cv, b, k, inverse))
