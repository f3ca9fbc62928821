"""Big-integer reference of b2f_fixed_base_mul_dev (csrc/b2f_fixed_base.hip) on tests/msm_ref.py.

The bases are known multiples [b] G of the generator, so the expected output for scalar s is
gen_mul(s b mod r): no Python double-and-add. recode() is the kernel's signed-digit recoding
restated in integers and partial_sums() the multiples of B its accumulator passes through, low
window first; the device tests use them to aim scalars at the recoding's carries and at the
additions where the accumulator equals the addend."""
import group_ntt_ref as gn
import msm_ref as mr


def expected(form, scalars, base_multiple):
    """[[s] B for s in scalars] for B = [base_multiple] G on the form's curve (affine, None: the
    identity)."""
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    return gn.gen_mul_many(cv, [s * base_multiple % r for s in scalars])


def recode(s, c, windows):
    """Signed digits d_w, low window first, with s = sum d_w 2^(w c) and -2^(c-1) < d_w <= 2^(c-1):
    t = (the window's bits) + carry; t > 2^(c-1) gives t - 2^c and a carry. Raises if a carry
    leaves the top window (it cannot for s < 2^(windows c - 1))."""
    assert 0 <= s < 1 << (windows * c)
    half, carry, out = 1 << (c - 1), 0, []
    for w in range(windows):
        t = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        carry = 1 if t > half else 0
        out.append(t - (carry << c))
    if carry:
        raise OverflowError("the recoding of %x carries out of window %d" % (s, windows - 1))
    return out


def value(digits, c):
    return sum(d << (w * c) for w, d in enumerate(digits))


def partial_sums(digits, c):
    """(window, accumulator multiple before the addition, addend multiple) for every non-zero
    digit, as integers (not reduced)."""
    acc, out = 0, []
    for w, d in enumerate(digits):
        if d:
            out.append((w, acc, d << (w * c)))
            acc += d << (w * c)
    return out


def meets(s, c, windows, r):
    """The set of {"double", "cancel"} events the accumulation of scalar s passes through on a
    base of order r: an addend equal or opposite to a non-identity accumulator."""
    ev = set()
    for _, acc, add in partial_sums(recode(s, c, windows), c):
        if acc % r == 0:
            continue  # the identity accumulator: its own branch, met by every scalar
        if (acc - add) % r == 0:
            ev.add("double")
        if (acc + add) % r == 0:
            ev.add("cancel")
    return ev


def doubling_scalar(c, windows, r):
    """A scalar < r whose last addition is P + P: s = 2 d 2^((windows-1) c) - r, the top digit d
    chosen so that the lower windows sum to d 2^(..) - r, of magnitude below the top window's
    unit."""
    unit = 1 << ((windows - 1) * c)
    d = (r + unit // 2) // unit  # the nearest: |d unit - r| <= unit / 2
    s = 2 * d * unit - r
    assert 0 < s < r and abs(d * unit - r) < unit
    return s
