// b2f_fieldprobe.hip -- diagnostics library only (libb2f_diag.so): one field primitive of
// b2f_field.h per lane on operands the caller chooses, for tests/test_gpu_field.py, which
// compares every result with Python integers. Not declared in include/b2f.h and not linked into
// libb2f.so.
//
//   int b2f_debug_field_op(field, op, a, b, n, out, flags)
//     field   0 pallas Fp, 1 BN254 Fr
//     op      B2F_FOP_* below
//     a, b    host, n elements of four little-endian u64 limbs each, used as the eight words
//             given (no form conversion: what a Montgomery-form op needs the caller passes in
//             Montgomery form)
//     out     host, n x 4 limbs; flags: host, n words: 1, or inv_safegcd's `ok`; 2 where the
//             kernel met a zero operand of an inverse (result zero, the inverse not called)
// It allocates, copies, runs one lane per element on the null stream and synchronises.
// B2F_ERR_ARG, nothing launched: a null pointer, n = 0 or n > 65,536, an unknown field or op,
// an operand >= p (the wide reduction excepted: it takes any two 256-bit integers), a zero `a`
// for an inverse (inv<F> does not terminate on 0 or on p).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/b2f.h"
#include "b2f_field.h"
#include "b2f_transcript.h"

namespace b2f {
namespace {

using namespace field;

enum : uint32_t {
  B2F_FOP_MUL = 0,       // the product the kernels call
  B2F_FOP_MUL_COMBA = 1,
  B2F_FOP_MUL_CIOS = 2,
  B2F_FOP_ADD = 3,
  B2F_FOP_SUB = 4,
  B2F_FOP_FROM_U32 = 5,  // of a's low word
  B2F_FOP_TO_MONT = 6,
  B2F_FOP_TO_CANONICAL = 7,
  B2F_FOP_POW = 8,       // a ^ (b's low word)
  B2F_FOP_INV = 9,
  B2F_FOP_INV_KALISKI = 10,
  B2F_FOP_INV_SAFEGCD = 11,
  B2F_FOP_INV_FERMAT = 12,
  B2F_FOP_COUNT = 13,
  // apart from the primitives above, whose operands are field elements: (a + b 2^256) mod p,
  // canonical, of any two 256-bit integers (b2f_transcript.h: a challenge from a 64-byte digest)
  B2F_FOP_REDUCE_WIDE = 32
};
__host__ __device__ inline bool is_inverse_op(uint32_t op) { return op >= B2F_FOP_INV && op <= B2F_FOP_INV_FERMAT; }

template <class F>
__global__ __launch_bounds__(64) void field_op_kernel(const uint64_t* a, const uint64_t* b, uint32_t n,
                                                      uint32_t op, uint64_t* out, uint32_t* flags) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const Fe x = load(a + 4ull * g), y = load(b + 4ull * g);
  Fe r = fe_zero();
  uint32_t flag = 1;
  if (is_inverse_op(op) && is_zero(x)) {  // the host refuses these; never reach inv<F> with 0
    flag = 2;
  } else {
    switch (op) {
      case B2F_FOP_MUL: r = mul<F>(x, y); break;
      case B2F_FOP_MUL_COMBA: r = mul_comba<F>(x, y); break;
      case B2F_FOP_MUL_CIOS: r = mul_cios<F>(x, y); break;
      case B2F_FOP_ADD: r = add<F>(x, y); break;
      case B2F_FOP_SUB: r = sub<F>(x, y); break;
      case B2F_FOP_FROM_U32: r = from_u32<F>(x.w[0]); break;
      case B2F_FOP_TO_MONT: r = to_mont<F>(x); break;
      case B2F_FOP_TO_CANONICAL: r = to_canonical<F>(x); break;
      case B2F_FOP_POW: r = fe_pow<F>(x, y.w[0]); break;
      case B2F_FOP_INV: r = inv<F>(x); break;
      case B2F_FOP_INV_KALISKI: r = inv_kaliski<F>(x); break;
      case B2F_FOP_INV_SAFEGCD: {
        bool ok = false;
        r = inv_safegcd<F>(x, ok);
        flag = ok ? 1u : 0u;
        break;
      }
      case B2F_FOP_INV_FERMAT: r = inv_fermat<F>(x); break;
      case B2F_FOP_REDUCE_WIDE: r = transcript::reduce_wide<F>(x, y); break;
      default: flag = 0; break;
    }
  }
  store(out + 4ull * g, r);
  flags[g] = flag;
}

// 0 for x = 0, 1 for 0 < x < p, 2 for x >= p
template <class F>
int classify(const uint64_t* x) {
  bool zero = true, below = false;  // below: x < p
  for (int i = 7; i >= 0; i--) {
    const uint32_t w = (uint32_t)(x[i >> 1] >> (32 * (i & 1)));
    if (w) zero = false;
    if (w != F::P[i]) {
      below = w < F::P[i];
      break;
    }
  }
  for (int i = 0; i < 4; i++)
    if (x[i]) zero = false;
  return zero ? 0 : below ? 1 : 2;
}

template <class F>
int field_op(uint32_t op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, uint32_t* flags) {
  for (size_t i = 0; i < n && op != B2F_FOP_REDUCE_WIDE; i++) {
    const int ca = classify<F>(a + 4 * i), cb = classify<F>(b + 4 * i);
    if (ca == 2 || cb == 2) return B2F_ERR_ARG;
    if (is_inverse_op(op) && ca == 0) return B2F_ERR_ARG;
  }
  const size_t bytes = 32 * n;
  uint64_t* d = nullptr;  // a | b | out | flags
  if (hipMalloc(&d, 3 * bytes + 4 * n) != hipSuccess) return B2F_ERR_HIP;
  uint64_t *da = d, *db = d + 4 * n, *dout = d + 8 * n;
  uint32_t* dflags = reinterpret_cast<uint32_t*>(d + 12 * n);
  int rc = B2F_OK;
  if (hipMemcpy(da, a, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(db, b, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dout, 0, bytes + 4 * n) != hipSuccess)
    rc = B2F_ERR_HIP;
  if (rc == B2F_OK) {
    hipLaunchKernelGGL(field_op_kernel<F>, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, 0, da, db, (uint32_t)n,
                       op, dout, dflags);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(flags, dflags, 4 * n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = B2F_ERR_HIP;
  }
  (void)hipFree(d);
  return rc;
}

}  // namespace
}  // namespace b2f

extern "C" B2F_API int b2f_debug_field_op(uint32_t field, uint32_t op, const uint64_t* a, const uint64_t* b,
                                          size_t n, uint64_t* out, uint32_t* flags) {
  if (!a || !b || !out || !flags || n == 0 || n > 65536 || field > 1 ||
      (op >= b2f::B2F_FOP_COUNT && op != b2f::B2F_FOP_REDUCE_WIDE))
    return B2F_ERR_ARG;
  return field ? b2f::field_op<b2f::field::Bn254>(op, a, b, n, out, flags)
               : b2f::field_op<b2f::field::Pallas>(op, a, b, n, out, flags);
}
