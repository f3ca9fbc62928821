"""Plain-integer model of b2f_msm_cells_dev's front end (csrc/b2f_msm.hip), with nothing imported
from the package: what scalar a column descriptor cuts from a u32 cell, how many windows a column
of `bits` bits has at window width c, and the signed-digit recoding of one cell.

A column is (offset, avail, shift, bits): scalar i is (cells[offset + i] >> shift) & (2^bits - 1)
for i < avail and zero from there to len. At width c it has ceil((bits + 1) / c) windows: the
field's bits and one more for the recoding carry. A digit above 2^(c-1) becomes digit - 2^c and
the next window gets the 2^c back; exactly 2^(c-1) stays as it is."""

NUM_ADVICE, NUM_FIXED = 10, 17
HALO2_INDEX = [7, 8, 9, 1, 2, 0, 3, 4, 5, 6]  # b2f_halo2_column_index


def windows(bits, c):
    return -(-(bits + 1) // c)


def scalar(cell, shift, bits):
    return (cell >> shift) & ((1 << bits) - 1)


def recode(value, bits, c):
    """The signed digits of a value below 2^bits, lowest window first."""
    assert 0 <= value < (1 << bits)
    half, out, carry = 1 << (c - 1), [], 0
    for w in range(windows(bits, c)):
        raw = ((value >> (w * c)) & ((1 << c) - 1)) + carry
        if raw > half:
            out.append(raw - (1 << c))
            carry = 1
        else:
            out.append(raw)
            carry = 0
    assert carry == 0, "the top window carried out"
    return out


def digit_count(cols, ln, c):
    """What a call recodes: len digits per window of every column."""
    return ln * sum(windows(bits, c) for _, _, _, bits in cols)


def column_scalars(cells, col, ln):
    """The len scalars of one column, as Python ints; cells: a flat sequence of u32."""
    offset, avail, shift, bits = col
    return [scalar(int(cells[offset + i]), shift, bits) if i < avail else 0 for i in range(ln)]


def advice_columns(total_rows, row_begin, usable_rows):
    """b2f_advice_cell_columns: entry HALO2_INDEX[i] describes a_i."""
    avail = 0 if row_begin >= total_rows else min(usable_rows, total_rows - row_begin)
    out = [None] * NUM_ADVICE
    for i in range(NUM_ADVICE):
        out[HALO2_INDEX[i]] = (i * total_rows + row_begin, avail, 0, 32)
    return out


def fixed_columns(total_rows, row_begin, usable_rows):
    """b2f_fixed_cell_columns: the selector bits, then k_0."""
    avail = 0 if row_begin >= total_rows else min(usable_rows, total_rows - row_begin)
    return [(row_begin, avail, c, 1) for c in range(16)] + [(row_begin, avail, 16, 16)]
