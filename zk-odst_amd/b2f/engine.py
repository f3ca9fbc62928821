"""Engine: one b2f_ctx on one HIP device, plus torch-allocated device trace buffers.

PyTorch is plumbing here (device memory, the stream handle); the work is the HIP kernels
behind include/b2f.h.
"""
import builtins  # the tensor-level opening calls take a `len` argument, as the ABI names it
import ctypes
import os

import numpy as np

from . import _lib
from .layout import INPUT_DTYPE, as_inputs, offsets as layout_offsets


def _vp(x):
    return ctypes.c_void_p(int(x))


def _np_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


_hip = None


def hip_runtime():
    """The HIP runtime this process (torch and libb2f.so) uses, for the one call torch does not
    order for us (copy_h2d_async)."""
    global _hip
    if _hip is None:
        import torch

        path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        _hip = ctypes.CDLL(path if os.path.exists(path) else "libamdhip64.so")
        _hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_int, ctypes.c_void_p]
        _hip.hipMemcpyAsync.restype = ctypes.c_int
    return _hip


def copy_h2d_async(dst, src, stream):
    """dst (device tensor) <- src (page-locked host tensor, same bytes) as hipMemcpyAsync on
    `stream`, the stream the library's launches go to: ordered before them. torch's own
    non_blocking copy (dst.copy_(src, non_blocking=True) under that stream) was measured NOT to
    be: tools/hasher_race.py (profiles/r03f_hasher_race.txt) -- 3 of 4 runs of 2^14 messages read
    a stale t counter in every step-0 input (49,152 wrong digests), 0 with this call, 0 with a
    host synchronize, 0 with blocking copies. The caller keeps src alive until the copy is done
    (the HIP call is invisible to torch's host allocator)."""
    nbytes = src.numel() * src.element_size()
    if nbytes != dst.numel() * dst.element_size():
        raise _lib.B2FError(_lib.ERR_ARG, "copy_h2d_async: %d bytes into %d"
                            % (nbytes, dst.numel() * dst.element_size()))
    rc = hip_runtime().hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 1, stream)
    if rc:
        raise _lib.B2FError(_lib.ERR_HIP, "hipMemcpyAsync returned %d" % rc)


class Engine:
    """Wraps b2f_create/b2f_destroy and the fill/eval entry points."""

    def __init__(self, device=0, diag=False, lib_path=None):
        """diag=True binds the diagnostics build (libb2f_diag.so); lib_path an explicit build
        of the same ABI (A/B runs). The default is the product library."""
        self.lib = _lib.load(diag=diag, path=lib_path)
        self.diag = bool(diag or lib_path)
        self.device = int(device)
        self.injecting = False  # debug_inject: the hook is on
        self.ctx = self.lib.b2f_create(self.device)
        if not self.ctx:
            raise _lib.B2FError(_lib.ERR_HIP, "b2f_create(%d) failed (no such HIP device?)" % device)

    def close(self):
        if self.ctx:
            self.lib.b2f_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        _lib.check(self.ctx, rc, self.lib)

    # ---------------------------------------------------------------- host-pointer calls
    def fill_host(self, inputs):
        """inputs: INPUT_DTYPE records. Returns (advice[10, R] u32, fixed[R] u32,
        h_out[n, 8] u64, offsets[n+1])."""
        inputs = as_inputs(inputs)
        off = layout_offsets(inputs)
        total = int(off[-1])
        adv = np.empty((_lib.NUM_ADVICE, total), dtype=np.uint32)
        fixed = np.empty(total, dtype=np.uint32)
        h_out = np.empty((len(inputs), 8), dtype=np.uint64)
        self._check(self.lib.b2f_fill(self.ctx, _np_ptr(inputs), len(inputs), _np_ptr(adv),
                                      _np_ptr(fixed), _np_ptr(h_out)))
        return adv, fixed, h_out, off

    def eval_host(self, adv, fixed, off):
        adv = np.ascontiguousarray(adv, dtype=np.uint32)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        rep = _lib.EvalReport()
        self._check(self.lib.b2f_eval(self.ctx, _np_ptr(adv), _np_ptr(fixed), _np_ptr(off),
                                      len(off) - 1, adv.shape[1], ctypes.byref(rep)))
        return rep.as_dict()

    # ---------------------------------------------------------------- device-pointer calls
    def fill_dev(self, d_in, n, d_off, total_rows, d_adv, d_fixed, d_h_out, stream=0):
        self._check(self.lib.b2f_fill_dev(self.ctx, _vp(d_in), n, _vp(d_off), int(total_rows),
                                          _vp(d_adv), _vp(d_fixed),
                                          _vp(d_h_out) if d_h_out else None, _vp(stream)))

    def eval_dev(self, d_adv, d_fixed, d_off, n, total_rows, d_report, stream=0):
        self._check(self.lib.b2f_eval_dev(self.ctx, _vp(d_adv), _vp(d_fixed), _vp(d_off), n,
                                          int(total_rows), _vp(d_report), _vp(stream)))

    def fill_eval_dev(self, d_in, n, d_off, total_rows, d_adv, d_fixed, d_h_out, d_report,
                      stream=0, flags=0):
        """b2f_fill_eval_dev_ex; flags=_lib.FIXED_RESIDENT states that d_fixed already holds this
        row map's fixed column (see include/b2f.h: the library checks its own record too). A
        library built before that entry point (lib_path) gets the plain call, flags dropped."""
        if not hasattr(self.lib, "b2f_fill_eval_dev_ex"):
            self._check(self.lib.b2f_fill_eval_dev(self.ctx, _vp(d_in), n, _vp(d_off),
                                                   int(total_rows), _vp(d_adv), _vp(d_fixed),
                                                   _vp(d_h_out) if d_h_out else None,
                                                   _vp(d_report), _vp(stream)))
            return
        self._check(self.lib.b2f_fill_eval_dev_ex(self.ctx, _vp(d_in), n, _vp(d_off),
                                                  int(total_rows), _vp(d_adv), _vp(d_fixed),
                                                  _vp(d_h_out) if d_h_out else None,
                                                  _vp(d_report), int(flags), _vp(stream)))

    def fill_fixed_dev(self, d_off, n, total_rows, d_fixed, stream=0):
        """Keygen structure: the fixed column from the row map alone (b2f_fill_fixed_dev)."""
        self._check(self.lib.b2f_fill_fixed_dev(self.ctx, _vp(d_off), int(n), int(total_rows),
                                                _vp(d_fixed), _vp(stream)))

    def debug_inject(self, row=None, col=0, mask=0):
        """Test hook: XOR `mask` into cell (row, col) (col 10 = fixed) as the fused path assigns
        it; row=None turns it off."""
        r = 2**64 - 1 if row is None else int(row)
        self._check(self.lib.b2f_debug_inject(self.ctx, r, int(col), int(mask) & 0xffffffff))
        self.injecting = row is not None

    def chain_inputs_dev(self, d_h_prev, d_blocks, d_t, d_f, rounds, n, d_out, stream=0):
        self._check(self.lib.b2f_chain_inputs_dev(self.ctx, _vp(d_h_prev), _vp(d_blocks), _vp(d_t),
                                                  _vp(d_f), int(rounds), int(n), _vp(d_out),
                                                  _vp(stream)))

    def export_fp_dev(self, d_adv, total_rows, row_begin, nrows, form, d_out, out_rows,
                      stream=0):
        self._check(self.lib.b2f_export_fp_dev(self.ctx, _vp(d_adv), int(total_rows),
                                               int(row_begin), int(nrows), int(form),
                                               _vp(d_out), int(out_rows), _vp(stream)))

    def export_fixed_fp_dev(self, d_fixed, total_rows, row_begin, nrows, form, d_out, out_rows,
                            stream=0):
        self._check(self.lib.b2f_export_fixed_fp_dev(self.ctx, _vp(d_fixed), int(total_rows),
                                                     int(row_begin), int(nrows), int(form),
                                                     _vp(d_out), int(out_rows), _vp(stream)))

    def lookup_columns_dev(self, d_adv, total_rows, d_row_begin, n_circuits, usable_rows, theta,
                           beta, gamma, form, d_out, out_rows, d_first_bad, stream=0):
        """b2f_lookup_columns_dev; theta/beta/gamma are Python ints (canonical Fp)."""
        lim = [(ctypes.c_uint64 * 4)(*[(int(v) >> (64 * k)) & (2**64 - 1) for k in range(4)])
               for v in (theta, beta, gamma)]
        self._check(self.lib.b2f_lookup_columns_dev(
            self.ctx, _vp(d_adv), int(total_rows), _vp(d_row_begin), int(n_circuits),
            int(usable_rows), lim[0], lim[1], lim[2], int(form), _vp(d_out), int(out_rows),
            _vp(d_first_bad), _vp(stream)))

    def spread_table_dev(self, usable_rows, form, d_out, out_rows, stream=0):
        self._check(self.lib.b2f_spread_table_dev(self.ctx, int(usable_rows), int(form), _vp(d_out),
                                                  int(out_rows), _vp(stream)))

    def spread_table(self, usable_rows, form=_lib.FP_MONTGOMERY, device="cuda:0", stream=None):
        """The spread table's three prover columns (tag, dense, spread): int64 tensor
        [3, usable_rows, 4] of field elements in `form` (b2f_spread_table_dev)."""
        import torch

        out = torch.empty((3, int(usable_rows), 4), dtype=torch.int64, device=device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.spread_table_dev(usable_rows, form, out.data_ptr(), int(usable_rows), s)
        return out

    def permutation_columns_dev(self, d_adv, total_rows, h_offsets, k, usable_rows, omega, delta,
                                beta, gamma, chunk_len, form, d_sigma, d_z, out_rows, stream=0):
        """b2f_permutation_columns_dev; h_offsets: host u64 row map of the circuit's instances,
        omega/delta/beta/gamma Python ints (canonical)."""
        off = np.ascontiguousarray(h_offsets, dtype=np.uint64)
        lim = [(ctypes.c_uint64 * 4)(*[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)])
               for v in (omega, delta, beta, gamma)]
        self._check(self.lib.b2f_permutation_columns_dev(
            self.ctx, _vp(d_adv), int(total_rows), _np_ptr(off), len(off) - 1, int(k),
            int(usable_rows), lim[0], lim[1], lim[2], lim[3], int(chunk_len), int(form),
            _vp(d_sigma) if d_sigma else None, _vp(d_z), int(out_rows), _vp(stream)))

    def permutation_columns_batch_dev(self, d_adv, total_rows, h_offsets, h_circuit_first, k,
                                      usable_rows, omega, delta, beta, gamma, chunk_len, form, d_z,
                                      out_rows, stream=0):
        """b2f_permutation_columns_batch_dev; h_offsets: host u64 row map of the instances,
        h_circuit_first: the circuits' instance boundaries (n_circuits + 1 of them),
        omega/delta/beta/gamma Python ints (canonical)."""
        off = np.ascontiguousarray(h_offsets, dtype=np.uint64)
        first = np.ascontiguousarray(h_circuit_first, dtype=np.uint64)
        lim = [(ctypes.c_uint64 * 4)(*[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)])
               for v in (omega, delta, beta, gamma)]
        self._check(self.lib.b2f_permutation_columns_batch_dev(
            self.ctx, _vp(d_adv), int(total_rows), _np_ptr(off), len(off) - 1, _np_ptr(first),
            max(len(first) - 1, 0), int(k), int(usable_rows), lim[0], lim[1], lim[2], lim[3],
            int(chunk_len), int(form), _vp(d_z), int(out_rows), _vp(stream)))

    def permutation_sigma_dev(self, h_offsets, k, omega, delta, form, d_sigma, out_rows, stream=0):
        """b2f_permutation_sigma_dev (keygen: the sigma columns alone); omega/delta Python ints."""
        off = np.ascontiguousarray(h_offsets, dtype=np.uint64)
        lim = [(ctypes.c_uint64 * 4)(*[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)])
               for v in (omega, delta)]
        self._check(self.lib.b2f_permutation_sigma_dev(
            self.ctx, _np_ptr(off), len(off) - 1, int(k), lim[0], lim[1], int(form), _vp(d_sigma),
            int(out_rows), _vp(stream)))

    def ntt_columns_dev(self, d_in, in_rows, in_len, n_cols, k, omega, shift, direction, form,
                        d_out, out_rows, stream=0):
        """b2f_ntt_columns_dev; omega/shift are Python ints (canonical)."""
        lim = [(ctypes.c_uint64 * 4)(*[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)])
               for v in (omega, shift)]
        self._check(self.lib.b2f_ntt_columns_dev(
            self.ctx, _vp(d_in), int(in_rows), int(in_len), int(n_cols), int(k), lim[0], lim[1],
            int(direction), int(form), _vp(d_out), int(out_rows), _vp(stream)))

    def ntt_columns(self, cols, k, inverse=False, shift=1, in_len=None, form=_lib.FP_MONTGOMERY,
                    out=None, stream=None):
        """NTT of every column of `cols`, a contiguous int64 [n_cols, rows, 4] tensor of field
        elements in `form`, over the 2^k domain of the form's field: forward (coefficients to
        evaluations on the coset shift <omega>; rows in_len .. 2^k - 1 count as zero) or inverse.
        Returns int64 [n_cols, 2^k, 4] (`out`, when given: contiguous int64 [n_cols, rows >= 2^k,
        4], rows past 2^k untouched) -- see b2f_ntt_columns_dev."""
        import torch

        from . import field

        if cols.dim() != 3 or cols.shape[2] != 4 or cols.dtype != torch.int64 \
                or not cols.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "ntt_columns: cols must be contiguous int64 [n_cols, rows, 4]")
        n_cols, rows = int(cols.shape[0]), int(cols.shape[1])
        n = 1 << int(k)
        in_len = min(rows, n) if in_len is None else int(in_len)
        if out is None:
            out = torch.empty((n_cols, n, 4), dtype=torch.int64, device=cols.device)
        if out.dim() != 3 or out.shape[0] != n_cols or out.shape[2] != 4 \
                or out.dtype != torch.int64 or not out.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "ntt_columns: out must be contiguous int64 [n_cols, rows, 4]")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.ntt_columns_dev(cols.data_ptr(), rows, in_len, n_cols, k,
                             field.omega(field.of_form(form), int(k)), shift,
                             _lib.NTT_INVERSE if inverse else _lib.NTT_FORWARD, form,
                             out.data_ptr(), int(out.shape[1]), s)
        return out

    # ---------------------------------------------------------------- quotient terms
    @staticmethod
    def _limbs(*vals):
        return [(ctypes.c_uint64 * 4)(*[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)])
                for v in vals]

    def lagrange_selectors_dev(self, k, usable_rows, form, d_out, out_rows, stream=0):
        self._check(self.lib.b2f_lagrange_selectors_dev(self.ctx, int(k), int(usable_rows), int(form),
                                                        _vp(d_out), int(out_rows), _vp(stream)))

    def quotient_gates_dev(self, k, ext_k, d_advice, d_fixed, rows, y, d_h_in, d_h_out, form, stream=0):
        """b2f_quotient_gates_dev; y is a Python int (canonical), d_h_in 0 or None for a zero
        accumulator."""
        lim = self._limbs(y)
        self._check(self.lib.b2f_quotient_gates_dev(
            self.ctx, int(k), int(ext_k), _vp(d_advice), _vp(d_fixed), int(rows), lim[0],
            _vp(d_h_in) if d_h_in else None, _vp(d_h_out), int(form), _vp(stream)))

    def quotient_permutation_dev(self, k, ext_k, usable_rows, d_l, d_advice, d_sigma, d_z, chunk_len,
                                 rows, omega_ext, shift, delta, beta, gamma, y, d_h_in, d_h_out, form,
                                 stream=0):
        """b2f_quotient_permutation_dev; omega_ext/shift/delta/beta/gamma/y are Python ints
        (canonical), d_h_in 0 or None for a zero accumulator."""
        lim = self._limbs(omega_ext, shift, delta, beta, gamma, y)
        self._check(self.lib.b2f_quotient_permutation_dev(
            self.ctx, int(k), int(ext_k), int(usable_rows), _vp(d_l), _vp(d_advice), _vp(d_sigma),
            _vp(d_z), int(chunk_len), int(rows), lim[0], lim[1], lim[2], lim[3], lim[4], lim[5],
            _vp(d_h_in) if d_h_in else None, _vp(d_h_out), int(form), _vp(stream)))

    def quotient_lookup_dev(self, k, ext_k, d_l, d_lookup, rows, beta, gamma, y, d_h_in, d_h_out, form,
                            stream=0):
        """b2f_quotient_lookup_dev; beta/gamma/y are Python ints (canonical)."""
        lim = self._limbs(beta, gamma, y)
        self._check(self.lib.b2f_quotient_lookup_dev(
            self.ctx, int(k), int(ext_k), _vp(d_l), _vp(d_lookup), int(rows), lim[0], lim[1], lim[2],
            _vp(d_h_in) if d_h_in else None, _vp(d_h_out), int(form), _vp(stream)))

    def quotient_divide_dev(self, k, ext_k, omega_ext, shift, d_h_in, d_h_out, form, stream=0):
        """b2f_quotient_divide_dev; omega_ext/shift are Python ints (canonical)."""
        lim = self._limbs(omega_ext, shift)
        self._check(self.lib.b2f_quotient_divide_dev(
            self.ctx, int(k), int(ext_k), lim[0], lim[1], _vp(d_h_in), _vp(d_h_out), int(form),
            _vp(stream)))

    @staticmethod
    def _cols(name, t, n_cols, min_rows):
        import torch

        if t.dim() != 3 or t.shape[0] != n_cols or t.shape[1] < min_rows or t.shape[2] != 4 \
                or t.dtype != torch.int64 or not t.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "%s must be contiguous int64 [%d, rows >= %d, 4]"
                                % (name, n_cols, min_rows))

    def _h(self, name, h, ext_k):
        import torch

        if h.dim() != 2 or h.shape[0] < (1 << ext_k) or h.shape[1] != 4 or h.dtype != torch.int64 \
                or not h.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "%s must be contiguous int64 [rows >= 2^ext_k, 4]" % name)

    def lagrange_selectors(self, k, usable_rows, form=_lib.FP_MONTGOMERY, device="cuda:0", stream=None):
        """l_0, l_last, l_active in the Lagrange basis: int64 [3, 2^k, 4] in `form`
        (b2f_lagrange_selectors_dev)."""
        import torch

        out = torch.empty((3, 1 << int(k), 4), dtype=torch.int64, device=device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.lagrange_selectors_dev(k, usable_rows, form, out.data_ptr(), 1 << int(k), s)
        return out

    def extend_columns(self, cols, k, ext_k, shift, form=_lib.FP_MONTGOMERY, stream=None):
        """Lagrange-form columns over 2^k rows (int64 [n_cols, rows >= 2^k, 4]) to their
        evaluations on the extended coset shift <omega_ext>: int64 [n_cols, 2^ext_k, 4]. The
        inverse NTT with shift 1, then the forward one on the coset with in_len = 2^k."""
        coeff = self.ntt_columns(cols, k, inverse=True, form=form, stream=stream)
        return self.ntt_columns(coeff, ext_k, shift=shift, in_len=1 << int(k), form=form, stream=stream)

    def quotient_gates(self, k, ext_k, advice, fixed, y, h=None, out=None, form=_lib.FP_MONTGOMERY,
                       stream=None):
        """The 74 custom-gate terms folded into h (b2f_quotient_gates_dev). advice [10, rows, 4]
        (halo2 column order, as export_fp writes them) and fixed [17, rows, 4] (as export_fixed_fp
        writes them): extended-coset columns of one stride rows >= 2^ext_k, int64 in `form`; h and
        out as in quotient_permutation. The gates come first in halo2's order: start h here."""
        import torch

        rows = int(advice.shape[1]) if advice.dim() == 3 else 0
        for name, t, nc in (("advice", advice, _lib.NUM_ADVICE), ("fixed", fixed, _lib.NUM_FIXED_FP)):
            self._cols("quotient_gates: " + name, t, nc, 1 << int(ext_k))
            if int(t.shape[1]) != rows:
                raise _lib.B2FError(_lib.ERR_ARG, "quotient_gates: the blocks must share one stride")
        if h is not None:
            self._h("quotient_gates: h", h, ext_k)
        if out is None:
            out = h if h is not None else torch.empty((1 << int(ext_k), 4), dtype=torch.int64,
                                                      device=advice.device)
        self._h("quotient_gates: out", out, ext_k)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.quotient_gates_dev(k, ext_k, advice.data_ptr(), fixed.data_ptr(), rows, y,
                                h.data_ptr() if h is not None else 0, out.data_ptr(), form, s)
        return out

    def quotient_permutation(self, k, ext_k, usable_rows, l, advice, sigma, z, chunk_len, shift, beta,
                             gamma, y, h=None, out=None, form=_lib.FP_MONTGOMERY, stream=None):
        """The permutation terms folded into h (b2f_quotient_permutation_dev). l [3, rows, 4],
        advice [10, rows, 4], sigma [8, rows, 4], z [ceil(8 / chunk_len), rows, 4]: extended-coset
        columns of one stride rows >= 2^ext_k, int64 in `form`. h: the accumulator so far ([rows >=
        2^ext_k, 4]) or None for zero; out: where the result goes (default: h itself, in place, or
        a new [2^ext_k, 4] tensor). The domain's omega_ext and the field's delta are the library's
        (b2f.field); shift is the caller's. Returns the result tensor."""
        import torch

        from . import field

        rows = int(l.shape[1]) if l.dim() == 3 else 0
        sets = (8 + int(chunk_len) - 1) // max(int(chunk_len), 1)
        for name, t, nc in (("l", l, 3), ("advice", advice, 10), ("sigma", sigma, 8), ("z", z, sets)):
            self._cols("quotient_permutation: " + name, t, nc, 1 << int(ext_k))
            if int(t.shape[1]) != rows:
                raise _lib.B2FError(_lib.ERR_ARG, "quotient_permutation: the blocks must share one stride")
        if h is not None:
            self._h("quotient_permutation: h", h, ext_k)
        if out is None:
            out = h if h is not None else torch.empty((1 << int(ext_k), 4), dtype=torch.int64, device=l.device)
        self._h("quotient_permutation: out", out, ext_k)
        f = field.of_form(form)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.quotient_permutation_dev(k, ext_k, usable_rows, l.data_ptr(), advice.data_ptr(),
                                      sigma.data_ptr(), z.data_ptr(), chunk_len, rows,
                                      field.omega(f, int(ext_k)), shift, field.delta(f), beta, gamma, y,
                                      h.data_ptr() if h is not None else 0, out.data_ptr(), form, s)
        return out

    def quotient_lookup(self, k, ext_k, l, lookup, beta, gamma, y, h=None, out=None,
                        form=_lib.FP_MONTGOMERY, stream=None):
        """The lookup terms folded into h (b2f_quotient_lookup_dev). l [3, rows, 4], lookup
        [5, rows, 4] (A, S, A', S', z extended); h and out as in quotient_permutation."""
        import torch

        rows = int(l.shape[1]) if l.dim() == 3 else 0
        for name, t, nc in (("l", l, 3), ("lookup", lookup, 5)):
            self._cols("quotient_lookup: " + name, t, nc, 1 << int(ext_k))
            if int(t.shape[1]) != rows:
                raise _lib.B2FError(_lib.ERR_ARG, "quotient_lookup: the blocks must share one stride")
        if h is not None:
            self._h("quotient_lookup: h", h, ext_k)
        if out is None:
            out = h if h is not None else torch.empty((1 << int(ext_k), 4), dtype=torch.int64, device=l.device)
        self._h("quotient_lookup: out", out, ext_k)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.quotient_lookup_dev(k, ext_k, l.data_ptr(), lookup.data_ptr(), rows, beta, gamma, y,
                                 h.data_ptr() if h is not None else 0, out.data_ptr(), form, s)
        return out

    def quotient_divide(self, k, ext_k, shift, h, out=None, form=_lib.FP_MONTGOMERY, stream=None):
        """h / (X^n - 1) on the extended coset (b2f_quotient_divide_dev): updates h in place, or
        writes `out` when given. Returns the result tensor."""
        import torch

        from . import field

        self._h("quotient_divide: h", h, ext_k)
        if out is None:
            out = h
        self._h("quotient_divide: out", out, ext_k)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.quotient_divide_dev(k, ext_k, field.omega(field.of_form(form), int(ext_k)), shift,
                                 h.data_ptr(), out.data_ptr(), form, s)
        return out

    # ---------------------------------------------------------------- evaluations and openings
    @staticmethod
    def _elems(vals):
        """Python ints as a uint64 [len, 4] host array of canonical little-endian limbs."""
        try:
            raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
        except OverflowError:
            raise _lib.B2FError(_lib.ERR_ARG, "a field element is negative or above 2^256")
        return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()

    def poly_eval_dev(self, d_cols, rows, len_, n_cols, points, queries, form, d_out, stream=0):
        """b2f_poly_eval_dev; points: Python ints (canonical), queries: (column, point index)
        pairs."""
        pts = self._elems(points)
        qs = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, 2)
        self._check(self.lib.b2f_poly_eval_dev(
            self.ctx, _vp(d_cols), int(rows), int(len_), int(n_cols), _np_ptr(pts), len(pts), _np_ptr(qs),
            len(qs), int(form), _vp(d_out), _vp(stream)))

    def poly_combine_dev(self, d_cols, rows, len_, n_cols, combos, form, d_out, out_rows, stream=0):
        """b2f_poly_combine_dev; combos: one list of (column, scalar int) terms per output."""
        first = np.zeros(len(combos) + 1, dtype=np.uint32)
        for o, terms in enumerate(combos):
            first[o + 1] = first[o] + len(terms)
        col = np.array([t[0] for terms in combos for t in terms] + [0], dtype=np.uint32)
        scal = self._elems([t[1] for terms in combos for t in terms] + [0])
        self._check(self.lib.b2f_poly_combine_dev(
            self.ctx, _vp(d_cols), int(rows), int(len_), int(n_cols), _np_ptr(first), _np_ptr(col),
            _np_ptr(scal), len(combos), int(form), _vp(d_out), int(out_rows), _vp(stream)))

    def kate_divide_dev(self, d_cols, rows, len_, n_cols, point_lists, form, d_out, out_rows, stream=0):
        """b2f_kate_divide_dev; point_lists: one list of Python ints (canonical) per column."""
        first = np.zeros(len(point_lists) + 1, dtype=np.uint32)
        for c, pts in enumerate(point_lists):
            first[c + 1] = first[c] + len(pts)
        pts = self._elems([z for lst in point_lists for z in lst] + [0])
        self._check(self.lib.b2f_kate_divide_dev(
            self.ctx, _vp(d_cols), int(rows), int(len_), int(n_cols), _np_ptr(first), _np_ptr(pts),
            int(form), _vp(d_out), int(out_rows), _vp(stream)))

    @staticmethod
    def _coeff_cols(name, t):
        import torch

        if t.dim() != 3 or t.shape[2] != 4 or t.dtype != torch.int64 or not t.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "%s must be contiguous int64 [n_cols, rows, 4]" % name)
        return int(t.shape[0]), int(t.shape[1])

    def poly_eval(self, cols, points, queries, len=None, form=_lib.FP_MONTGOMERY, stream=None):
        """Evaluations of coefficient columns (b2f_poly_eval_dev). cols: int64 [n_cols, rows, 4] in
        `form`, the first `len` rows (default: all) of each a polynomial's coefficients; points:
        Python ints; queries: (column, point index) pairs in any order. Returns int64
        [n_queries, 4] in `form`."""
        import torch

        n_cols, rows = self._coeff_cols("poly_eval: cols", cols)
        n = rows if len is None else int(len)
        qs = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, 2)
        out = torch.empty((qs.shape[0], 4), dtype=torch.int64, device=cols.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.poly_eval_dev(cols.data_ptr(), rows, n, n_cols, points, qs, form, out.data_ptr(), s)
        return out

    def poly_combine(self, cols, combos, len=None, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """Linear combinations of coefficient columns (b2f_poly_combine_dev): output o is the sum
        of scalar * cols[column] over the (column, scalar) terms of combos[o] (none: zeros), on the
        first `len` rows. Returns int64 [n_out, len, 4] (`out`, when given: [n_out, rows >= len, 4],
        rows past len untouched)."""
        import torch

        n_cols, rows = self._coeff_cols("poly_combine: cols", cols)
        n = rows if len is None else int(len)
        if out is None:
            out = torch.empty((builtins.len(combos), n, 4), dtype=torch.int64, device=cols.device)
        n_out, out_rows = self._coeff_cols("poly_combine: out", out)
        if n_out != builtins.len(combos):
            raise _lib.B2FError(_lib.ERR_ARG, "poly_combine: out must hold one column per output")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.poly_combine_dev(cols.data_ptr(), rows, n, n_cols, combos, form, out.data_ptr(), out_rows, s)
        return out

    def kate_divide(self, cols, point_lists, len=None, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """halo2's kate_division of column c by (X - z) for each z of point_lists[c] in turn
        (b2f_kate_divide_dev), on the first `len` rows. Returns int64 [n_cols, len, 4] (`out`, when
        given: [n_cols, rows >= len, 4], rows past len untouched)."""
        import torch

        n_cols, rows = self._coeff_cols("kate_divide: cols", cols)
        n = rows if len is None else int(len)
        if builtins.len(point_lists) != n_cols:
            raise _lib.B2FError(_lib.ERR_ARG, "kate_divide: one point list per column")
        if out is None:
            out = torch.empty((n_cols, n, 4), dtype=torch.int64, device=cols.device)
        n_out, out_rows = self._coeff_cols("kate_divide: out", out)
        if n_out != n_cols:
            raise _lib.B2FError(_lib.ERR_ARG, "kate_divide: out must hold one column per input")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.kate_divide_dev(cols.data_ptr(), rows, n, n_cols, point_lists, form, out.data_ptr(), out_rows, s)
        return out

    # ---------------------------------------------------------------- commitments
    def msm_dev(self, d_scalars, rows, len_, n_cols, d_bases, n_bases, form, d_out, stream=0):
        """b2f_msm_dev: d_out[c] = sum_i scalar[c][i] base[i] for n_cols columns, as affine points
        in base-field Montgomery form (b2f/curve.py packs and unpacks them)."""
        self._check(self.lib.b2f_msm_dev(self.ctx, _vp(d_scalars), int(rows), int(len_), int(n_cols),
                                         _vp(d_bases), int(n_bases), int(form), _vp(d_out), _vp(stream)))

    def msm(self, scalars, bases, len=None, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """Commitments of columns (b2f_msm_dev). scalars: int64 [n_cols, rows, 4] in `form`, the
        first `len` rows (default: all) of each committed; bases: int64 [n_bases >= len, 8] affine
        points of the form's curve (curve.pack_points). Returns int64 [n_cols, 8] affine points, the
        identity all zeros."""
        import torch

        n_cols, rows = self._coeff_cols("msm: scalars", scalars)
        n = rows if len is None else int(len)
        if bases.dim() != 2 or bases.shape[1] != 8 or bases.dtype != torch.int64 or not bases.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "msm: bases must be contiguous int64 [n_bases, 8]")
        if out is None:
            out = torch.empty((n_cols, 8), dtype=torch.int64, device=scalars.device)
        if out.dim() != 2 or tuple(out.shape) != (n_cols, 8) or out.dtype != torch.int64 or not out.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "msm: out must be contiguous int64 [n_cols, 8]")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.msm_dev(scalars.data_ptr(), rows, n, n_cols, bases.data_ptr(), int(bases.shape[0]), form,
                     out.data_ptr(), s)
        return out

    def msm_cells_dev(self, d_cells, n_cells, cols, len_, d_tail, tail_rows, d_bases, n_bases, form, d_out,
                      stream=0):
        """b2f_msm_cells_dev: commitments of columns cut from u32 cells. cols: a list of (offset,
        avail, shift, bits) or a ctypes array of _lib.CellColumn (copied by the call)."""
        arr = cols if isinstance(cols, ctypes.Array) else _lib.cell_columns(cols)
        self._check(self.lib.b2f_msm_cells_dev(self.ctx, _vp(d_cells), int(n_cells), arr, len(arr), int(len_),
                                               _vp(d_tail), int(tail_rows), _vp(d_bases), int(n_bases),
                                               int(form), _vp(d_out), _vp(stream)))

    def msm_cells(self, cells, cols, bases, len, tail=None, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """Commitments of columns where they lie (b2f_msm_cells_dev). cells: a contiguous int32 /
        uint32 tensor (any shape: indexed flat); cols: a list of (offset, avail, shift, bits), scalar
        i of a column being (cells[offset + i] >> shift) & (2^bits - 1) for i < avail and zero from
        there to `len`; tail: int64 [n_cols, tail_rows, 4] full scalars in `form` multiplying bases
        len .. len + tail_rows - 1 (the blinding rows), or None; bases: int64 [n_bases >= len +
        tail_rows, 8]. Returns int64 [n_cols, 8] affine points, the identity all zeros."""
        import torch

        if cells.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not cells.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "msm_cells: cells must be a contiguous int32 / uint32 tensor")
        if bases.dim() != 2 or bases.shape[1] != 8 or bases.dtype != torch.int64 or not bases.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "msm_cells: bases must be contiguous int64 [n_bases, 8]")
        n_cols = builtins.len(cols)
        tail_rows = 0
        if tail is not None:
            if tail.dim() != 3 or tail.shape[0] != n_cols or tail.shape[2] != 4 or tail.dtype != torch.int64 \
                    or not tail.is_contiguous():
                raise _lib.B2FError(_lib.ERR_ARG, "msm_cells: tail must be contiguous int64 [n_cols, tail_rows, 4]")
            tail_rows = int(tail.shape[1])
        if out is None:
            out = torch.empty((n_cols, 8), dtype=torch.int64, device=cells.device)
        if out.dim() != 2 or tuple(out.shape) != (n_cols, 8) or out.dtype != torch.int64 or not out.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "msm_cells: out must be contiguous int64 [n_cols, 8]")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.msm_cells_dev(cells.data_ptr(), cells.numel(), cols, len, tail.data_ptr() if tail_rows else 0,
                           tail_rows, bases.data_ptr(), int(bases.shape[0]), form, out.data_ptr(), s)
        return out

    # ---------------------------------------------------------------- IPA opening rounds
    def ipa_powers_dev(self, x, len_, form, d_b, stream=0):
        """b2f_ipa_powers_dev: d_b[i] = x^i for i < len, in `form`; x a Python int (canonical)."""
        self._check(self.lib.b2f_ipa_powers_dev(self.ctx, _np_ptr(self._elems([x])), int(len_), int(form),
                                                _vp(d_b), _vp(stream)))

    def ipa_round_dev(self, d_p, d_b, d_g, len_, form, d_lr, d_values, stream=0):
        """b2f_ipa_round_dev: the round's cross terms (L, R) and inner products (value_l, value_r)."""
        self._check(self.lib.b2f_ipa_round_dev(self.ctx, _vp(d_p), _vp(d_b), _vp(d_g), int(len_), int(form),
                                               _vp(d_lr), _vp(d_values), _vp(stream)))

    def ipa_fold_dev(self, d_p, d_b, d_g, len_, u, form, stream=0):
        """b2f_ipa_fold_dev: the three collapses in place; u a Python int (canonical, non-zero)."""
        self._check(self.lib.b2f_ipa_fold_dev(self.ctx, _vp(d_p), _vp(d_b), _vp(d_g), int(len_),
                                              _np_ptr(self._elems([u])), int(form), _vp(stream)))

    @staticmethod
    def _ipa_vectors(name, p, b, g, n):
        import torch

        for what, t, w in (("p", p, 4), ("b", b, 4), ("g", g, 8)):
            if t.dim() != 2 or t.shape[1] != w or t.dtype != torch.int64 or not t.is_contiguous():
                raise _lib.B2FError(_lib.ERR_ARG, "%s: %s must be contiguous int64 [rows, %d]" % (name, what, w))
            if int(t.shape[0]) < n:
                raise _lib.B2FError(_lib.ERR_ROWS, "%s: %s holds fewer than len = %d rows" % (name, what, n))

    def ipa_powers(self, x, len, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """b = (1, x, x^2, ..) (b2f_ipa_powers_dev): int64 [len, 4] in `form`; x a Python int."""
        import torch

        n = int(len)
        if out is None:
            out = torch.empty((n, 4), dtype=torch.int64, device="cuda:%d" % self.device)
        if out.dim() != 2 or out.shape[1] != 4 or out.dtype != torch.int64 or not out.is_contiguous() \
                or int(out.shape[0]) < n:
            raise _lib.B2FError(_lib.ERR_ARG, "ipa_powers: out must be contiguous int64 [rows >= len, 4]")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.ipa_powers_dev(x, n, form, out.data_ptr(), s)
        return out

    def ipa_round(self, p, b, g, len=None, form=_lib.FP_MONTGOMERY, stream=None):
        """One round's cross terms and inner products (b2f_ipa_round_dev). p, b: int64 [rows, 4]
        scalars in `form`; g: int64 [rows, 8] affine points (curve.pack_points); the first `len`
        rows (default: all of p) are the round's vectors. Returns (int64 [2, 8] = (L, R) affine,
        the identity all zeros; int64 [2, 4] = (value_l, value_r) in `form`)."""
        import torch

        n = int(p.shape[0]) if len is None else int(len)
        self._ipa_vectors("ipa_round", p, b, g, n)
        lr = torch.empty((2, 8), dtype=torch.int64, device=p.device)
        values = torch.empty((2, 4), dtype=torch.int64, device=p.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.ipa_round_dev(p.data_ptr(), b.data_ptr(), g.data_ptr(), n, form, lr.data_ptr(), values.data_ptr(), s)
        return lr, values

    def ipa_fold(self, p, b, g, u, len=None, form=_lib.FP_MONTGOMERY, stream=None):
        """The round's collapses in place on rows below len / 2 (b2f_ipa_fold_dev); u a Python int,
        the round's challenge. Rows from len / 2 on are left as they are."""
        import torch

        n = int(p.shape[0]) if len is None else int(len)
        self._ipa_vectors("ipa_fold", p, b, g, n)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.ipa_fold_dev(p.data_ptr(), b.data_ptr(), g.data_ptr(), n, u, form, s)

    # ---------------------------------------------------------------- transcript, one-call opening
    def transcript_init_dev(self, d_state, stream=0):
        """b2f_transcript_init_dev: the empty transcript into the 32 words at d_state."""
        self._check(self.lib.b2f_transcript_init_dev(self.ctx, _vp(d_state), _vp(stream)))

    def transcript_absorb_points_dev(self, d_state, d_points, n, form, stream=0):
        """b2f_transcript_absorb_points_dev: common_point of n affine points, in order."""
        self._check(self.lib.b2f_transcript_absorb_points_dev(self.ctx, _vp(d_state), _vp(d_points), int(n),
                                                              int(form), _vp(stream)))

    def transcript_absorb_scalars_dev(self, d_state, d_scalars, n, form, stream=0):
        """b2f_transcript_absorb_scalars_dev: common_scalar of n scalars in `form`, in order."""
        self._check(self.lib.b2f_transcript_absorb_scalars_dev(self.ctx, _vp(d_state), _vp(d_scalars), int(n),
                                                               int(form), _vp(stream)))

    def transcript_squeeze_dev(self, d_state, form, d_challenge, stream=0):
        """b2f_transcript_squeeze_dev: squeeze_challenge, four canonical limbs to d_challenge."""
        self._check(self.lib.b2f_transcript_squeeze_dev(self.ctx, _vp(d_state), int(form), _vp(d_challenge),
                                                        _vp(stream)))

    def ipa_open_dev(self, d_p, d_b, d_g, len_, u_point, w_point, d_z, d_rand, d_state, form, d_lr, d_u, d_cf,
                     stream=0):
        """b2f_ipa_open_dev: the whole opening loop queued on `stream`. u_point, w_point: packed host
        points, 8 uint64 limbs each (curve.pack_points)."""
        pts = []
        for base in (u_point, w_point):
            limbs = np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)
            if limbs.size != 8:
                raise _lib.B2FError(_lib.ERR_ARG, "ipa_open: U and W are 8 limbs each")
            pts.append(limbs)
        self._check(self.lib.b2f_ipa_open_dev(self.ctx, _vp(d_p), _vp(d_b), _vp(d_g), int(len_), _np_ptr(pts[0]),
                                              _np_ptr(pts[1]), _vp(d_z), _vp(d_rand), _vp(d_state), int(form),
                                              _vp(d_lr), _vp(d_u), _vp(d_cf), _vp(stream)))

    @staticmethod
    def _rows(name, what, t, width, min_rows=1):
        import torch

        if t.dim() != 2 or t.shape[1] != width or t.dtype != torch.int64 or not t.is_contiguous() \
                or int(t.shape[0]) < min_rows:
            raise _lib.B2FError(_lib.ERR_ARG, "%s: %s must be contiguous int64 [rows >= %d, %d]"
                                % (name, what, min_rows, width))

    @staticmethod
    def _state(name, state):
        import torch

        if state.dim() != 1 or state.shape[0] != _lib.TRANSCRIPT_BYTES // 8 or state.dtype != torch.int64 \
                or not state.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "%s: state must be contiguous int64 [32]" % name)

    def transcript_init(self, stream=None):
        """A new transcript (b2f_transcript_init_dev): the state, int64 [32] on this engine's GPU, whose
        words are the ABI of include/b2f.h (h, t, the block buffer, the buffered bytes)."""
        import torch

        state = torch.empty(_lib.TRANSCRIPT_BYTES // 8, dtype=torch.int64, device="cuda:%d" % self.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.transcript_init_dev(state.data_ptr(), s)
        return state

    def transcript_absorb_points(self, state, points, form=_lib.FP_MONTGOMERY, stream=None):
        """common_point of every row of points, int64 [n, 8] affine points of the form's curve
        (curve.pack_points), in order. An identity row reports B2F_ERR_FIELD at sync."""
        import torch

        self._state("transcript_absorb_points", state)
        self._rows("transcript_absorb_points", "points", points, 8)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.transcript_absorb_points_dev(state.data_ptr(), points.data_ptr(), int(points.shape[0]), form, s)

    def transcript_absorb_scalars(self, state, scalars, form=_lib.FP_MONTGOMERY, stream=None):
        """common_scalar of every row of scalars, int64 [n, 4] in `form`, in order."""
        import torch

        self._state("transcript_absorb_scalars", state)
        self._rows("transcript_absorb_scalars", "scalars", scalars, 4)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.transcript_absorb_scalars_dev(state.data_ptr(), scalars.data_ptr(), int(scalars.shape[0]), form, s)

    def transcript_squeeze(self, state, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """squeeze_challenge: int64 [4], the canonical limbs of a challenge of the form's scalar field
        (whatever the form), on the device: what ipa_open takes as z."""
        import torch

        self._state("transcript_squeeze", state)
        if out is None:
            out = torch.empty(4, dtype=torch.int64, device=state.device)
        if out.dim() != 1 or out.shape[0] != 4 or out.dtype != torch.int64 or not out.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "transcript_squeeze: out must be contiguous int64 [4]")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.transcript_squeeze_dev(state.data_ptr(), form, out.data_ptr(), s)
        return out

    def ipa_open(self, p, b, g, U, W, z, rand, state, f, len=None, form=_lib.FP_MONTGOMERY, stream=None):
        """The whole opening in one queued call (b2f_ipa_open_dev): every round's blinded L_j, R_j,
        the challenges u_j squeezed from `state` on the device, the folds, c and f, with no host step
        between rounds. p, b, g: as for ipa_round, folded in place; U, W: (x, y) pairs of Python ints
        or 8 packed limbs; z: int64 [4] canonical limbs on the device (transcript_squeeze); rand:
        int64 [2 k, 4] in `form`, (l_rand_j, r_rand_j) per round; f: int64 [4], the starting f in
        `form`. Returns (lr int64 [k, 2, 8], u int64 [k, 4] canonical, cf int64 [2, 4] = (c, f) in
        `form`)."""
        import torch

        from . import curve

        n = int(p.shape[0]) if len is None else int(len)
        self._ipa_vectors("ipa_open", p, b, g, n)
        k = max(n.bit_length() - 1, 1)
        self._state("ipa_open", state)
        self._rows("ipa_open", "rand", rand, 4, 2 * k)
        for what, t in (("z", z), ("f", f)):
            if t.dim() != 1 or t.shape[0] != 4 or t.dtype != torch.int64 or not t.is_contiguous():
                raise _lib.B2FError(_lib.ERR_ARG, "ipa_open: %s must be contiguous int64 [4]" % what)
        cv = curve.of_form(form)
        U, W = [curve.pack_points(cv, [pt])[0] if isinstance(pt, tuple) and builtins.len(pt) == 2 else pt
                for pt in (U, W)]
        lr = torch.empty((k, 2, 8), dtype=torch.int64, device=p.device)
        u = torch.empty((k, 4), dtype=torch.int64, device=p.device)
        cf = torch.empty((2, 4), dtype=torch.int64, device=p.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        if s == torch.cuda.current_stream().cuda_stream:
            cf[1].copy_(f)  # the starting f, ordered on the call's stream
        else:
            with torch.cuda.stream(torch.cuda.ExternalStream(s)):
                cf[1].copy_(f)
        self.ipa_open_dev(p.data_ptr(), b.data_ptr(), g.data_ptr(), n, U, W, z.data_ptr(), rand.data_ptr(),
                          state.data_ptr(), form, lr.data_ptr(), u.data_ptr(), cf.data_ptr(), s)
        return lr, u, cf

    # ---------------------------------------------------------------- group NTT (g -> g_lagrange)
    def group_ntt_dev(self, d_in, k, omega, direction, form, d_out, stream=0):
        """b2f_group_ntt_dev: the transform of 2^k affine points; omega a Python int (canonical)."""
        self._check(self.lib.b2f_group_ntt_dev(self.ctx, _vp(d_in), int(k), self._limbs(omega)[0],
                                               int(direction), int(form), _vp(d_out), _vp(stream)))

    def group_ntt(self, points, k, inverse=False, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """The group NTT of the first 2^k rows of `points`, int64 [rows >= 2^k, 8] affine points of
        the form's curve (curve.pack_points), over the 2^k domain of the form's scalar field
        (omega from b2f.field.omega): forward, or inverse (with the n^-1). Returns int64 [2^k, 8]
        affine points, the identity all zeros; out=points transforms in place (rows past 2^k
        untouched) -- see b2f_group_ntt_dev. Both tensors must be on this engine's GPU.
        _lib.group_ntt_plan counts the inverse's scalar multiplications, n + (n / 2)(k - 1); the
        forward direction performs n fewer."""
        import torch

        from . import field

        n = 1 << int(k)
        if points.dim() != 2 or points.shape[1] != 8 or points.dtype != torch.int64 or not points.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "group_ntt: points must be contiguous int64 [rows, 8]")
        if int(points.shape[0]) < n:
            raise _lib.B2FError(_lib.ERR_ROWS, "group_ntt: points holds fewer than 2^k = %d rows" % n)
        if out is None:
            out = torch.empty((n, 8), dtype=torch.int64, device=points.device)
        if out.dim() != 2 or out.shape[1] != 8 or out.dtype != torch.int64 or not out.is_contiguous() \
                or int(out.shape[0]) < n:
            raise _lib.B2FError(_lib.ERR_ARG, "group_ntt: out must be contiguous int64 [rows >= 2^k, 8]")
        for what, t in (("points", points), ("out", out)):
            if t.device.type != "cuda" or t.device.index != self.device:
                raise _lib.B2FError(_lib.ERR_ARG, "group_ntt: %s is on %s, not on cuda:%d"
                                    % (what, t.device, self.device))
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.group_ntt_dev(points.data_ptr(), k, field.omega(field.of_form(form), int(k)),
                           _lib.NTT_INVERSE if inverse else _lib.NTT_FORWARD, form, out.data_ptr(), s)
        return out

    def g_to_lagrange(self, g, k, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """halo2's g_to_lagrange: the Lagrange-basis points of the parameters' g over the 2^k
        domain, the bases of commit_lagrange (msm_cells, DeviceBatch.commit_advice): the inverse
        group NTT."""
        return self.group_ntt(g, k, inverse=True, form=form, out=out, stream=stream)

    # ---------------------------------------------------------------- fixed-base multiples, KZG set-up
    def fixed_base_mul_dev(self, base, d_scalars, len_, form, d_out, stream=0):
        """b2f_fixed_base_mul_dev: d_out[i] = [s_i] B. base: the packed host point, 8 uint64 limbs
        (curve.pack_points; all zero: the identity)."""
        limbs = np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)
        if limbs.size != 8:
            raise _lib.B2FError(_lib.ERR_ARG, "fixed_base_mul: the base is 8 limbs")
        self._check(self.lib.b2f_fixed_base_mul_dev(self.ctx, _np_ptr(limbs), _vp(d_scalars), int(len_),
                                                    int(form), _vp(d_out), _vp(stream)))

    def fixed_base_mul(self, scalars, base=None, form=_lib.FP_MONTGOMERY, out=None, stream=None):
        """Multiples of one point (b2f_fixed_base_mul_dev): out[i] = [scalars[i]] B. scalars: int64
        [len, 4] reduced scalars in `form`; base: None for the generator of the form's curve
        (curve.GENERATOR), an (x, y) pair of Python ints, or 8 packed limbs (curve.pack_points: the
        identity all zeros). Returns int64 [len, 8] affine points, the identity all zeros. The
        base's table is built on the first call with it and cached by the engine's context (four
        bases); _lib.fixed_base_plan reports its shape."""
        import torch

        from . import curve

        if scalars.dim() != 2 or scalars.shape[1] != 4 or scalars.dtype != torch.int64 or not scalars.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "fixed_base_mul: scalars must be contiguous int64 [len, 4]")
        n = int(scalars.shape[0])
        cv = curve.of_form(form)
        if base is None:
            base = curve.GENERATOR[cv]
        if isinstance(base, tuple) and builtins.len(base) == 2:
            base = curve.pack_points(cv, [base])[0]
        if out is None:
            out = torch.empty((n, 8), dtype=torch.int64, device=scalars.device)
        if out.dim() != 2 or out.shape[1] != 8 or out.dtype != torch.int64 or not out.is_contiguous() \
                or int(out.shape[0]) < n:
            raise _lib.B2FError(_lib.ERR_ARG, "fixed_base_mul: out must be contiguous int64 [rows >= len, 8]")
        for what, t in (("scalars", scalars), ("out", out)):
            if t.device.type != "cuda" or t.device.index != self.device:
                raise _lib.B2FError(_lib.ERR_ARG, "fixed_base_mul: %s is on %s, not on cuda:%d"
                                    % (what, t.device, self.device))
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self.fixed_base_mul_dev(base, scalars.data_ptr(), n, form, out.data_ptr(), s)
        return out

    def kzg_setup(self, k, tau, form=_lib.FP_BN254_MONTGOMERY, lagrange=True, stream=None):
        """halo2's UNSAFE KZG set-up, ParamsKZG::setup(k, rng) with the caller's tau in the place
        of the rng's: g[i] = [tau^i] G for i < 2^k (G: curve.GENERATOR of the form's curve) and
        g_lagrange = g_to_lagrange(g). Returns (g, g_lagrange), int64 [2^k, 8] each (g_lagrange is
        None with lagrange=False). It composes ipa_powers(tau, 2^k), fixed_base_mul and
        g_to_lagrange on `stream`.

        tau is known to the caller, so whoever holds it can forge openings: this is for tests,
        benches and development, exactly as ParamsKZG::setup is. A production caller loads the
        points of a ceremony instead and never calls this. [tau] G2 and the pairing are not built
        here."""
        n = 1 << int(k)
        powers = self.ipa_powers(int(tau), n, form=form, stream=stream)
        g = self.fixed_base_mul(powers, form=form, stream=stream)
        return g, (self.g_to_lagrange(g, k, form=form, stream=stream) if lagrange else None)

    def debug_curve_op(self, op, a, b, curve, za=None, zb=None):
        """Diagnostics build only (b2f_debug_curve_op): the base-field primitive or point operation
        `op` (a name of _lib.CURVE_OPS) on the device, one lane per element. Field ops: a, b uint64
        [n, 4]; point ops: a, b uint64 [n, 8] affine points and za, zb uint64 [n, 4] the z the
        operand is lifted to XYZZ with. curve: 0 Vesta, 1 BN254 G1. Returns (out, flags uint32 [n])."""
        idx = _lib.CURVE_OPS.index(op)
        w = 4 if idx < _lib.CURVE_FIELD_OPS else 8
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, w)
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, w)
        if len(a) != len(b):
            raise _lib.B2FError(_lib.ERR_ARG, "debug_curve_op: a and b differ in length")
        zs = []
        for z in (za, zb):
            if z is None:
                z = np.zeros((len(a), 4), dtype=np.uint64)
            z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
            if len(z) != len(a):
                raise _lib.B2FError(_lib.ERR_ARG, "debug_curve_op: z differs in length")
            zs.append(z)
        out = np.zeros_like(a)
        flags = np.zeros(len(a), dtype=np.uint32)
        rc = self.lib.b2f_debug_curve_op(int(curve), idx, _np_ptr(a), _np_ptr(b), _np_ptr(zs[0]),
                                         _np_ptr(zs[1]), len(a), _np_ptr(out), _np_ptr(flags))
        if rc != _lib.OK:
            raise _lib.B2FError(rc, "debug_curve_op(%s) refused or failed" % op)
        return out, flags

    def debug_eval_path(self):
        """Path of the last eval_dev call (device-synchronizing): 0 the fast clean-check pass
        found the trace clean, 1 it flagged something and the exact eval kernel reported, 2 no
        fast pass ran."""
        out = ctypes.c_uint32(0)
        self._check(self.lib.b2f_debug_eval_path(self.ctx, ctypes.byref(out)))
        return int(out.value)

    def debug_fused_path(self):
        """Kernel of the last fill_eval_dev call (host state, no synchronize): 0 the full one,
        1 the advice-only one (FIXED_RESIDENT honoured)."""
        out = ctypes.c_uint32(0)
        self._check(self.lib.b2f_debug_fused_path(self.ctx, ctypes.byref(out)))
        return int(out.value)

    def debug_field_op(self, op, a, b, field):
        """Diagnostics build only (b2f_debug_field_op): the field primitive `op` (a name of
        _lib.FIELD_OPS) on the device, one lane per element. a, b: uint64 [n, 4] host limbs, used as
        given; field: 0 pallas, 1 BN254. Returns (out uint64 [n, 4], flags uint32 [n])."""
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
        if len(a) != len(b):
            raise _lib.B2FError(_lib.ERR_ARG, "debug_field_op: a and b differ in length")
        out = np.zeros_like(a)
        flags = np.zeros(len(a), dtype=np.uint32)
        rc = self.lib.b2f_debug_field_op(int(field), _lib.FIELD_OPS.index(op), _np_ptr(a), _np_ptr(b),
                                         len(a), _np_ptr(out), _np_ptr(flags))
        if rc != _lib.OK:
            raise _lib.B2FError(rc, "debug_field_op(%s) refused or failed" % op)
        return out, flags

    def debug_reduce_wide(self, a, b, field):
        """Diagnostics build only (b2f_debug_field_op, op FIELD_OP_REDUCE_WIDE): (a + b 2^256) mod p on
        the device, canonical, one lane per pair. a, b: uint64 [n, 4] host limbs, ANY 256-bit integers
        (the two halves of a 64-byte digest); field: 0 pallas, 1 BN254. Returns out uint64 [n, 4]."""
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
        if len(a) != len(b):
            raise _lib.B2FError(_lib.ERR_ARG, "debug_reduce_wide: a and b differ in length")
        out = np.zeros_like(a)
        flags = np.zeros(len(a), dtype=np.uint32)
        rc = self.lib.b2f_debug_field_op(int(field), _lib.FIELD_OP_REDUCE_WIDE, _np_ptr(a), _np_ptr(b),
                                         len(a), _np_ptr(out), _np_ptr(flags))
        if rc != _lib.OK:
            raise _lib.B2FError(rc, "debug_reduce_wide refused or failed")
        return out

    def sync(self, stream=0):
        self._check(self.lib.b2f_sync(self.ctx, _vp(stream)))

    def set_timing(self, enable=True):
        self._check(self.lib.b2f_set_timing(self.ctx, 1 if enable else 0))

    def kernel_times(self):
        """{kernel: (total_ms, launches)} since set_timing(True) / the previous call."""
        k = int(self.lib.b2f_num_kernels())  # the library's count sizes the buffers
        if k != len(_lib.KERNEL_NAMES):
            raise _lib.B2FError(_lib.ERR_ARG, "library reports %d kernel kinds, binding knows %d"
                                % (k, len(_lib.KERNEL_NAMES)))
        tot = (ctypes.c_double * k)()
        cnt = (ctypes.c_uint32 * k)()
        self._check(self.lib.b2f_kernel_times(self.ctx, tot, cnt))
        return {name: (float(tot[i]), int(cnt[i])) for i, name in enumerate(_lib.KERNEL_NAMES)}


def permutation_mapping(rounds):
    """Keygen's permutation mapping of one instance: u32 [8, R] entries (c' << 29) | r'
    (b2f_permutation_mapping)."""
    lib = _lib.load()
    n = int(lib.b2f_permutation_mapping(int(rounds), None, 0))
    out = np.zeros(n, dtype=np.uint32)
    lib.b2f_permutation_mapping(int(rounds), _np_ptr(out), n)
    return out.reshape(8, -1)


def copy_constraints(rounds):
    """The copy constraints of one instance: u32 [count, 4] (dst_row, dst_col, src_row,
    src_col), instance-relative rows (b2f_copy_constraints)."""
    lib = _lib.load()
    n = int(lib.b2f_copy_constraints(int(rounds), None, 0))
    out = np.zeros((n, 4), dtype=np.uint32)
    lib.b2f_copy_constraints(int(rounds), _np_ptr(out), n)
    return out


def gate_queries():
    """The advice queries of the chip's sixteen gates: u32 [count, 2] (halo2 advice column,
    rotation), sorted by column then rotation (b2f_gate_queries)."""
    lib = _lib.load()
    n = int(lib.b2f_gate_queries(None, 0))
    out = np.zeros((n, 2), dtype=np.uint32)
    lib.b2f_gate_queries(_np_ptr(out), n)
    return out


def _cell_columns(fn, n, total_rows, row_begin, usable_rows):
    arr = (_lib.CellColumn * n)()
    if int(fn(int(total_rows), int(row_begin), int(usable_rows), arr)) != n:
        raise _lib.B2FError(_lib.ERR_ARG, "cell columns: total_rows %d is no multiple of 4 or usable_rows %d is 0"
                            % (total_rows, usable_rows))
    return [(int(d.offset), int(d.avail), int(d.shift), int(d.bits)) for d in arr]


def advice_cell_columns(total_rows, row_begin, usable_rows):
    """The ten (offset, avail, shift, bits) descriptors of one circuit's advice columns over the
    trace's advice block, in halo2 column order (b2f_advice_cell_columns)."""
    return _cell_columns(_lib.load().b2f_advice_cell_columns, _lib.NUM_ADVICE, total_rows, row_begin, usable_rows)


def fixed_cell_columns(total_rows, row_begin, usable_rows):
    """The seventeen descriptors of one circuit's fixed columns over the packed fixed column:
    selector bits 0..15, then k_0 (b2f_fixed_cell_columns)."""
    return _cell_columns(_lib.load().b2f_fixed_cell_columns, _lib.NUM_FIXED_FP, total_rows, row_begin, usable_rows)


class DeviceBatch:
    """A batch resident on one GPU: inputs, offsets, the trace and the outputs, as torch
    tensors (int32/int64 storage holding u32/u64 bit patterns)."""

    def __init__(self, inputs, device="cuda:0", total_rows=None):
        import torch

        self.torch = torch
        inputs = as_inputs(inputs)
        self.n = len(inputs)
        off = layout_offsets(inputs)
        self.offsets_host = off
        self.used_rows = int(off[-1])
        self.total_rows = int(total_rows) if total_rows is not None else self.used_rows
        if self.total_rows < self.used_rows or self.total_rows % 4:
            raise _lib.B2FError(_lib.ERR_ROWS, "total_rows %d (need >= %d, multiple of 4)"
                                % (self.total_rows, self.used_rows))
        dev = torch.device(device)
        raw = np.frombuffer(inputs.tobytes(), dtype=np.uint8)
        # synchronous (pageable) uploads: construction is not the hot path, and a later launch
        # on any stream sees them (see copy_h2d_async for the asynchronous form)
        self.inputs = torch.from_numpy(raw.copy()).to(dev)
        self.offsets = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        self.advice = torch.empty((_lib.NUM_ADVICE, self.total_rows), dtype=torch.int32, device=dev)
        self.fixed = torch.empty(self.total_rows, dtype=torch.int32, device=dev)
        self.h_out = torch.empty((self.n, 8), dtype=torch.int64, device=dev)
        self.report = torch.empty(_lib.REPORT_BYTES // 8, dtype=torch.int64, device=dev)
        self._fixed_seal = None

    def _seal(self, eng):
        """What must still hold at the next fill_evaluate for the fixed column to count as
        resident: the engine's context and the version counters of `fixed` and `offsets` (torch
        bumps a tensor's counter on every in-place write, through views too; reads leave it).
        None -- never resident -- for a diagnostics or lib_path engine, under the inject hook, or
        where the counters cannot be read."""
        if eng.diag or eng.injecting:
            return None
        try:
            return (eng.ctx, self.fixed.data_ptr(), self.fixed._version, self.offsets._version)
        except Exception:
            return None

    def invalidate_fixed(self):
        """Forget that `fixed` holds the keygen column: the next fill_evaluate writes it. For
        writers torch's version counter does not see (.data, a foreign holder of data_ptr(),
        DLPack)."""
        self._fixed_seal = None

    def fill(self, eng, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream().cuda_stream
        self._fixed_seal = None
        eng.fill_dev(self.inputs.data_ptr(), self.n, self.offsets.data_ptr(), self.total_rows,
                     self.advice.data_ptr(), self.fixed.data_ptr(), self.h_out.data_ptr(), s)
        self._fixed_seal = self._seal(eng)

    def evaluate(self, eng, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream().cuda_stream
        eng.eval_dev(self.advice.data_ptr(), self.fixed.data_ptr(), self.offsets.data_ptr(),
                     self.n, self.total_rows, self.report.data_ptr(), s)

    def fill_evaluate(self, eng, stream=None, fixed_resident=None):
        """Fused fill + eval (b2f_fill_eval_dev_ex): trace, h' and report in one pass.

        The fixed column is a function of the row map alone (keygen output), so a repeat call
        leaves it in place. fixed_resident=None decides that automatically: the call states
        B2F_FIXED_RESIDENT only if this batch's last fill / fill_evaluate ran on this same
        product engine with the inject hook off, and neither `fixed` nor `offsets` has been
        written through torch since (their version counters are unchanged). Everything else --
        a first call, another engine, a diagnostics or lib_path engine, the hook -- writes the
        whole trace. fixed_resident=False always does. Writes torch cannot see (.data, a
        foreign holder of data_ptr(), DLPack) are the caller's business: invalidate_fixed()."""
        s = stream if stream is not None else self.torch.cuda.current_stream().cuda_stream
        seal = self._seal(eng)
        resident = fixed_resident is None and seal is not None and seal == self._fixed_seal
        self._fixed_seal = None  # a call that raises leaves nothing resident
        eng.fill_eval_dev(self.inputs.data_ptr(), self.n, self.offsets.data_ptr(),
                          self.total_rows, self.advice.data_ptr(), self.fixed.data_ptr(),
                          self.h_out.data_ptr(), self.report.data_ptr(), s,
                          flags=_lib.FIXED_RESIDENT if resident else 0)
        self._fixed_seal = seal

    def export_fp(self, eng, row_begin=0, nrows=None, form=_lib.FP_MONTGOMERY, out=None,
                  stream=None):
        """Advice rows [row_begin, row_begin + nrows) as pallas Fp elements: int64 tensor
        [10 (halo2 column order), out_rows, 4] (u64 limb bit patterns). `out` may be a
        preallocated tensor of that shape (out_rows >= nrows)."""
        torch = self.torch
        nrows = self.total_rows - row_begin if nrows is None else int(nrows)
        if out is None:
            out = torch.empty((_lib.NUM_ADVICE, nrows, 4), dtype=torch.int64,
                              device=self.advice.device)
        if out.dim() != 3 or out.shape[0] != _lib.NUM_ADVICE or out.shape[2] != 4 \
                or out.dtype != torch.int64 or not out.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "export_fp: out must be contiguous int64 [10, rows, 4]")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        eng.export_fp_dev(self.advice.data_ptr(), self.total_rows, row_begin, nrows, form,
                          out.data_ptr(), out.shape[1], s)
        return out

    def export_fixed_fp(self, eng, row_begin=0, nrows=None, form=_lib.FP_MONTGOMERY, out=None,
                        stream=None):
        """Fixed rows [row_begin, row_begin + nrows) as the prover's fixed columns: int64 tensor
        [17 (selector bits 0..15, then k_0), out_rows, 4] of field elements in `form`
        (b2f_export_fixed_fp_dev). `out` may be a preallocated tensor of that shape (out_rows >=
        nrows; rows past nrows are left as they are)."""
        torch = self.torch
        nrows = self.total_rows - row_begin if nrows is None else int(nrows)
        if out is None:
            out = torch.empty((_lib.NUM_FIXED_FP, nrows, 4), dtype=torch.int64,
                              device=self.fixed.device)
        if out.dim() != 3 or out.shape[0] != _lib.NUM_FIXED_FP or out.shape[2] != 4 \
                or out.dtype != torch.int64 or not out.is_contiguous():
            raise _lib.B2FError(_lib.ERR_ARG, "export_fixed_fp: out must be contiguous int64 [17, rows, 4]")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        eng.export_fixed_fp_dev(self.fixed.data_ptr(), self.total_rows, row_begin, nrows, form,
                                out.data_ptr(), out.shape[1], s)
        return out

    def commit_advice(self, eng, row_begin, usable_rows, bases, tail=None, form=_lib.FP_MONTGOMERY,
                      stream=None):
        """Commitments of the advice columns of circuits cut from the trace, read where the fill
        left them (b2f_msm_cells_dev): halo2's commit_lagrange of each column against `bases`
        (g_lagrange: int64 [n_bases, 8]), the scalars being rows row_begin .. + usable_rows - 1 and
        then `tail` (int64 [n_columns, tail_rows, 4] in `form`: the blinding rows). row_begin: an
        int (10 points out), or a list of ints: all the circuits in one call, circuit c's halo2
        column h at output c * 10 + h. Returns int64 [10 * n_circuits, 8]."""
        begins = [row_begin] if isinstance(row_begin, (int, np.integer)) else list(row_begin)
        cols = []
        for rb in begins:
            cols += advice_cell_columns(self.total_rows, rb, usable_rows)
        return eng.msm_cells(self.advice, cols, bases, usable_rows, tail=tail, form=form, stream=stream)

    def commit_fixed(self, eng, row_begin, usable_rows, bases, form=_lib.FP_MONTGOMERY, stream=None):
        """Commitments of one circuit's seventeen fixed columns (keygen), read from the packed
        fixed column in export_fixed_fp's order. Returns int64 [17, 8]."""
        cols = fixed_cell_columns(self.total_rows, row_begin, usable_rows)
        return eng.msm_cells(self.fixed, cols, bases, usable_rows, form=form, stream=stream)

    def lookup_columns(self, eng, row_begin, usable_rows, theta, beta, gamma,
                       form=_lib.FP_MONTGOMERY, stream=None):
        """Lookup-argument prover columns for circuits starting at trace rows `row_begin`:
        (out int64 [n_circuits, 5 (A, S, A', S', z), usable_rows + 1, 4], first_bad int64
        [n_circuits]) -- see b2f_lookup_columns_dev."""
        torch = self.torch
        dev = self.advice.device
        rb = torch.tensor([int(r) for r in row_begin], dtype=torch.int64, device=dev)
        nc = len(row_begin)
        out = torch.empty((nc, 5, usable_rows + 1, 4), dtype=torch.int64, device=dev)
        bad = torch.empty(nc, dtype=torch.int64, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        eng.lookup_columns_dev(self.advice.data_ptr(), self.total_rows, rb.data_ptr(), nc,
                               usable_rows, theta, beta, gamma, form, out.data_ptr(),
                               usable_rows + 1, bad.data_ptr(), s)
        return out, bad

    def permutation_columns(self, eng, k, usable_rows, beta, gamma, chunk_len=3,
                            form=_lib.FP_MONTGOMERY, instances=None, sigma=True, stream=None):
        """Permutation-argument prover columns of the circuit holding instances
        [i0, i1) = `instances` (default: all) in a 2^k-row domain: (sigma int64 [8, 2^k, 4] or
        None, z int64 [sets, 2^k, 4] with rows 0..usable_rows written) -- see
        b2f_permutation_columns_dev. omega and delta come from the field of `form`."""
        from . import field

        torch = self.torch
        dev = self.advice.device
        i0, i1 = (0, self.n) if instances is None else instances
        off = self.offsets_host[i0:i1 + 1]
        f = field.of_form(form)
        n_rows = 1 << int(k)
        sets = (8 + chunk_len - 1) // chunk_len
        sig = torch.empty((8, n_rows, 4), dtype=torch.int64, device=dev) if sigma else None
        z = torch.empty((sets, n_rows, 4), dtype=torch.int64, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        eng.permutation_columns_dev(self.advice.data_ptr(), self.total_rows, off, k, usable_rows,
                                    field.omega(f, int(k)), field.delta(f), beta, gamma,
                                    chunk_len, form, sig.data_ptr() if sigma else 0,
                                    z.data_ptr(), n_rows, s)
        return sig, z

    def permutation_columns_batch(self, eng, k, usable_rows, beta, gamma, circuits, chunk_len=3,
                                  form=_lib.FP_MONTGOMERY, stream=None):
        """The permutation z columns of C circuits in one call, every circuit in its own 2^k-row
        domain under the same challenges: `circuits` = the instance boundaries [i_0, i_1, ...,
        i_C], circuit c holding instances [i_c, i_{c+1}). Returns z int64 [C, sets, 2^k, 4] with
        rows 0..usable_rows written, z[c] equal to permutation_columns(instances=(i_c, i_{c+1}),
        sigma=False)[1] -- see b2f_permutation_columns_batch_dev."""
        from . import field

        torch = self.torch
        first = [int(i) for i in circuits]
        f = field.of_form(form)
        n_rows = 1 << int(k)
        sets = (8 + chunk_len - 1) // chunk_len
        z = torch.empty((max(len(first) - 1, 0), sets, n_rows, 4), dtype=torch.int64,
                        device=self.advice.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        eng.permutation_columns_batch_dev(self.advice.data_ptr(), self.total_rows, self.offsets_host,
                                          first, k, usable_rows, field.omega(f, int(k)),
                                          field.delta(f), beta, gamma, chunk_len, form, z.data_ptr(),
                                          n_rows, s)
        return z

    def permutation_sigma(self, eng, k, form=_lib.FP_MONTGOMERY, instances=None, stream=None):
        """Keygen's sigma columns (int64 [8, 2^k, 4]) of the circuit holding instances
        [i0, i1) = `instances` (default: all): b2f_permutation_sigma_dev, the same columns
        permutation_columns returns, without a witness."""
        from . import field

        torch = self.torch
        i0, i1 = (0, self.n) if instances is None else instances
        off = self.offsets_host[i0:i1 + 1]
        f = field.of_form(form)
        n_rows = 1 << int(k)
        sig = torch.empty((8, n_rows, 4), dtype=torch.int64, device=self.advice.device)
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        eng.permutation_sigma_dev(off, k, field.omega(f, int(k)), field.delta(f), form, sig.data_ptr(),
                                  n_rows, s)
        return sig

    def report_dict(self):
        raw = self.report.cpu().numpy().view(np.uint64)
        rep = _lib.EvalReport.from_buffer_copy(raw.tobytes())
        return rep.as_dict()

    def host_trace(self):
        adv = self.advice.cpu().numpy().view(np.uint32)
        fixed = self.fixed.cpu().numpy().view(np.uint32)
        return adv, fixed

    def host_h_out(self):
        return self.h_out.cpu().numpy().view(np.uint64)
