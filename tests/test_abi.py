"""The C ABI library loads and exports every function include/b2f.h declares; the
host-only entry points (no GPU needed) behave as documented."""
import ctypes
import re
import struct

import numpy as np
import pytest

from conftest import ROOT, random_inputs


def declared_functions():
    src = open(ROOT + "/include/b2f.h").read()
    return re.findall(r"B2F_API\s+[\w\s\*]+?\b(b2f_\w+)\s*\(", src)


def test_all_declared_symbols_exported():
    import b2f
    from b2f import _lib

    lib = b2f.load()
    names = declared_functions()
    assert len(names) >= 15
    for name in names:
        assert hasattr(lib, name), name
    assert sorted(names) == sorted(n for n, _, _ in _lib.SIGNATURES)


def test_layout_rows_and_offsets(orc):
    import b2f

    for r in (0, 1, 4, 12, 1000):
        assert b2f.rows(r) == 228 + 416 * r == orc.rows(r)
    with pytest.raises(b2f.B2FError):
        b2f.rows((1 << 20) + 1)
    x = random_inputs(17, (0, 1, 4, 12), 21)
    ox = np.frombuffer(x.tobytes(), dtype=orc.INPUT_DTYPE).copy()
    assert np.array_equal(b2f.offsets(x), orc.offsets(ox))


def test_halo2_column_index():
    import b2f

    # table16.rs:281-294 allocation order: message_schedule (a_5), extras (a_3,a_4,a_6..a_9),
    # then the lookup inputs a_0, a_1, a_2
    assert [b2f.halo2_column_index(i) for i in range(10)] == [7, 8, 9, 1, 2, 0, 3, 4, 5, 6]
    assert b2f.halo2_column_index(10) == -1


def _eip152(rounds, h, m, t, f):
    return (struct.pack(">I", rounds) + struct.pack("<8Q", *h) + struct.pack("<16Q", *m)
            + struct.pack("<2Q", *t) + bytes([f]))


def test_parse_eip152(golden):
    import b2f

    k = golden["kat"]
    h = [int(w, 16) for w in k["h"]]
    m = [int(w, 16) for w in k["m"]]
    raw = _eip152(12, h, m, [3, 0], 1)
    assert len(raw) == 213
    rec = b2f.parse_eip152(raw)
    assert rec["rounds"] == 12 and rec["f"] == 1 and list(rec["t"]) == [3, 0]
    assert [int(v) for v in rec["h"]] == h and [int(v) for v in rec["m"]] == m
    with pytest.raises(b2f.B2FError) as e:
        b2f.parse_eip152(raw[:-1])
    assert e.value.code == 6
    with pytest.raises(b2f.B2FError):
        b2f.parse_eip152(raw[:-1] + b"\x02")  # EIP-152: f must be 0 or 1


def test_no_device_is_an_error_not_a_fallback():
    """Without a GPU the engine refuses to start: there is no CPU fallback path."""
    import torch

    import b2f

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(b2f.B2FError):
        b2f.Engine(0)


def test_null_context_calls_fail_cleanly():
    import b2f

    lib = b2f.load()
    assert lib.b2f_fill_dev(None, None, 0, None, 0, None, None, None, None) == 1
    assert lib.b2f_eval(None, None, None, None, 0, 0, None) == 1
    assert lib.b2f_last_error(None) == b"null context"


def test_missing_library_fails_loudly():
    """No fallback: without the HIP library every entry point raises (checked in a fresh
    interpreter so the loaded library of this session is not reused)."""
    import subprocess
    import sys

    code = ("import sys; sys.path.insert(0, %r)\n"
            "import b2f\nfrom b2f import _lib\n"
            "_lib.LIB_PATH = '/nonexistent/libb2f.so'\n"
            "try:\n    b2f.load()\nexcept OSError as e:\n    print('raised', 'not found' in str(e))\n"
            "try:\n    b2f.Engine(0)\nexcept OSError as e:\n    print('raised2')\n") % (ROOT + "/zk-odst_amd")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert "raised True" in out.stdout and "raised2" in out.stdout, out.stdout + out.stderr


def test_product_library_reads_no_environment():
    """the diagnostic kernel variants (selected by B2F_DIAG_* /
    B2F_FILL_WGS) live only in libb2f_diag.so; libb2f.so does not even contain the names, so
    no environment can swap a product kernel for a diagnostic one."""
    from b2f import _lib

    prod = open(_lib.LIB_PATH, "rb").read()
    diag = open(_lib.DIAG_LIB_PATH, "rb").read()
    for var in (b"B2F_DIAG_EVAL", b"B2F_DIAG_FILL", b"B2F_DIAG_FUSED", b"B2F_FILL_WGS",
                b"B2F_DIAG_NTT_PLAN", b"b2f_debug_field_op", b"b2f_debug_ntt_plan"):
        assert var not in prod, var
        assert var in diag, var
    lib = _lib.load(diag=True)
    for name, _, _ in _lib.SIGNATURES:
        assert hasattr(lib, name), name
    # the test hooks are exports of the diagnostics library alone
    prod_lib = _lib.load()
    for name, _, _ in _lib.DIAG_SIGNATURES:
        assert hasattr(lib, name), name
        assert not hasattr(prod_lib, name), name


def test_ntt_pass_plan_table():
    """The product's pass plan for every k (b2f_debug_ntt_plan, host only): one pass up to k = 10,
    then ceil(k / 8) passes of digits <= 8, non-increasing, differing by at most 1, summing to k.
    With B2F_DIAG_NTT_PLAN set, the export reports the forced plan or refuses as the call would."""
    import os

    from b2f import B2FError, _lib

    assert "B2F_DIAG_NTT_PLAN" not in os.environ
    for k in range(1, 29):
        l = _lib.debug_ntt_plan(k)
        assert len(l) == (1 if k <= 10 else -(-k // 8)), (k, l)
        assert sum(l) == k and all(1 <= d for d in l), (k, l)
        if k > 10:
            assert max(l) <= 8 and max(l) - min(l) <= 1 and l == sorted(l, reverse=True), (k, l)
    assert _lib.debug_ntt_plan(25) == [7, 6, 6, 6] and _lib.debug_ntt_plan(28) == [7, 7, 7, 7]
    for k in (0, 29):
        with pytest.raises(B2FError):
            _lib.debug_ntt_plan(k)
    try:
        os.environ["B2F_DIAG_NTT_PLAN"] = "3,3,3,2"
        assert _lib.debug_ntt_plan(11) == [3, 3, 3, 2]
        for k in (10, 12):  # the sum is not k
            with pytest.raises(B2FError) as e:
                _lib.debug_ntt_plan(k)
            assert e.value.code == _lib.ERR_ARG
        for bad, k in (("", 11), ("11", 11), ("6,5,", 11), ("6, 5", 11), ("0,8,3", 11), ("9,2", 11),
                       ("3,2,2,2,2", 11), ("5,5", 10), ("10", 10), ("6,5x", 11), ("-6,5", 11),
                       ("06,5", 11), ("8,8,8,8", 28 + 4)):
            os.environ["B2F_DIAG_NTT_PLAN"] = bad
            with pytest.raises(B2FError) as e:
                _lib.debug_ntt_plan(k)
            assert e.value.code == _lib.ERR_ARG, (bad, k)
        os.environ["B2F_DIAG_NTT_PLAN"] = "8,8,8,1"
        assert _lib.debug_ntt_plan(25) == [8, 8, 8, 1]
    finally:
        os.environ.pop("B2F_DIAG_NTT_PLAN", None)
    assert _lib.debug_ntt_plan(11) == [6, 5]


@pytest.mark.parametrize("rounds", [0, 1, 2, 12, 13])
def test_copy_constraints_match_oracle_structure(orc, rounds):
    """b2f_copy_constraints (the product's keygen copy list, host code) == the equality pairs
    the oracle's structure-mode synthesis records, in the same (synthesis) order -- the
    permutation argument's cycle order depends on it; count 24 + 576 rounds + 96."""
    import b2f

    got = b2f.copy_constraints(rounds)
    want = orc.copies(rounds)
    assert len(got) == 24 + 576 * rounds + 96 == len(want)
    assert np.array_equal(got, want)
    assert len(set(map(tuple, got[:, :2].tolist()))) == len(got)  # one copy per operand cell


def test_status_codes_match_the_header():
    """The ctypes binding's status codes and names are the header's #defines."""
    from b2f import _lib

    src = open(ROOT + "/include/b2f.h").read()
    codes = {m.group(1): int(m.group(2))
             for m in re.finditer(r"#define (B2F_(?:OK|ERR_\w+))\s+(\d+)", src)}
    assert codes["B2F_ERR_FIELD"] == 7
    assert {v: k for k, v in _lib.STATUS_NAMES.items()} == \
        {("OK" if k == "B2F_OK" else k): v for k, v in codes.items()}


def test_kernel_count_and_report_codes_match_the_header():
    """b2f_kernel_times writes b2f_num_kernels() entries, which is the header's
    B2F_NUM_KERNELS and the binding's KERNEL_NAMES; the report codes (incl. B2F_CODE_CHECK)
    are the header's."""
    import b2f
    from b2f import _lib

    src = open(ROOT + "/include/b2f.h").read()
    n = int(re.search(r"#define B2F_NUM_KERNELS\s+(\d+)", src).group(1))
    assert b2f.load().b2f_num_kernels() == n == len(_lib.KERNEL_NAMES)
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define B2F_(CODE_\w+)\s+(\d+)", src)}
    assert codes == {k: getattr(_lib, k) for k in codes} and codes["CODE_CHECK"] == 20
