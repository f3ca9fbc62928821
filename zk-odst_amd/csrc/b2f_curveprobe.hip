// b2f_curveprobe.hip -- diagnostics library only (libb2f_diag.so): one base-field primitive of
// b2f_field.h or one point operation of b2f_curve.h per lane on operands the caller chooses, for
// tests/test_gpu_curve_ops.py, which compares every result with Python integers. Not declared in
// include/b2f.h and not linked into libb2f.so.
//
//   int b2f_debug_curve_op(curve, op, a, b, za, zb, n, out, flags)
//     curve   0 Vesta (base field pasta Fq), 1 BN254 G1 (base field bn256::Fq)
//     op      B2F_COP_* below
//     field ops: a, b host, n elements of four little-endian u64 limbs, used as given (no form
//             conversion); za, zb ignored (may be null); out n x 4 limbs
//     point ops: a, b host, n affine points of 8 limbs (x, y in Montgomery form, (0, 0) the
//             identity); za, zb host, n Montgomery-form elements: the operand is lifted to XYZZ as
//             (x z^2, y z^3, z^2, z^3), so a test chooses accumulators that are not normalised
//             (z = 0: the operand becomes the identity whatever a is); out n x 8 limbs, the
//             result made affine on the device
//     flags   host, n words: 1, or the `ok` of the inversion the op ended with
// It allocates, copies, runs one lane per element on the null stream and synchronises.
// B2F_ERR_ARG, nothing launched: a null pointer, n = 0 or n > 65,536, an unknown curve or op, an
// operand word block >= p.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/b2f.h"
#include "b2f_curve.h"
#include "b2f_field.h"

namespace b2f {
namespace {

using namespace field;
using namespace curve;

enum : uint32_t {
  B2F_COP_MUL = 0,
  B2F_COP_ADD = 1,
  B2F_COP_SUB = 2,
  B2F_COP_TO_MONT = 3,
  B2F_COP_TO_CANONICAL = 4,
  B2F_COP_INV_SAFEGCD = 5,  // a = 0 gives 0
  B2F_COP_FIELD_END = 6,
  B2F_COP_MADD = 6,   // lift(a, za) + b (mixed)
  B2F_COP_PADD = 7,   // lift(a, za) + lift(b, zb) (full)
  B2F_COP_DBL = 8,    // 2 lift(a, za)
  B2F_COP_NEG = 9,    // -lift(a, za)
  B2F_COP_MDBL = 10,  // 2 a, a affine and not the identity (the identity is passed through)
  B2F_COP_COUNT = 11
};

template <class F>
__device__ Xyzz lift(const Affine& p, const Fe& z) {
  if (is_identity(p) || is_zero(z)) return xyzz_identity();
  Xyzz r;
  r.zz = mul<F>(z, z);
  r.zzz = mul<F>(r.zz, z);
  r.x = mul<F>(p.x, r.zz);
  r.y = mul<F>(p.y, r.zzz);
  return r;
}

template <class F>
__global__ __launch_bounds__(64) void curve_op_kernel(const uint64_t* a, const uint64_t* b, const uint64_t* za,
                                                      const uint64_t* zb, uint32_t n, uint32_t op, uint64_t* out,
                                                      uint32_t* flags) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  uint32_t flag = 1;
  if (op < B2F_COP_FIELD_END) {
    const Fe x = load(a + 4ull * g), y = load(b + 4ull * g);
    Fe r = fe_zero();
    switch (op) {
      case B2F_COP_MUL: r = mul<F>(x, y); break;
      case B2F_COP_ADD: r = add<F>(x, y); break;
      case B2F_COP_SUB: r = sub<F>(x, y); break;
      case B2F_COP_TO_MONT: r = to_mont<F>(x); break;
      case B2F_COP_TO_CANONICAL: r = to_canonical<F>(x); break;
      default: {
        bool ok = false;
        r = inv_safegcd<F>(x, ok);
        flag = ok ? 1u : 0u;
        break;
      }
    }
    store(out + 4ull * g, r);
  } else {
    const Affine p = load_affine(a + 8ull * g), q = load_affine(b + 8ull * g);
    const Xyzz P = lift<F>(p, load(za + 4ull * g));
    Xyzz r;
    switch (op) {
      case B2F_COP_MADD: r = madd<F>(P, q); break;
      case B2F_COP_PADD: r = curve::add<F>(P, lift<F>(q, load(zb + 4ull * g))); break;
      case B2F_COP_DBL: r = dbl<F>(P); break;
      case B2F_COP_NEG: r = neg<F>(P); break;
      default: r = is_identity(p) ? xyzz_identity() : mdbl<F>(p); break;
    }
    bool ok = true;
    store_affine(out + 8ull * g, to_affine<F>(r, ok));
    flag = ok ? 1u : 0u;
  }
  flags[g] = flag;
}

template <class F>
bool below_p(const uint64_t* x) {
  for (int i = 7; i >= 0; i--) {
    const uint32_t w = (uint32_t)(x[i >> 1] >> (32 * (i & 1)));
    if (w != F::P[i]) return w < F::P[i];
  }
  return false;
}

template <class F>
int curve_op(uint32_t op, const uint64_t* a, const uint64_t* b, const uint64_t* za, const uint64_t* zb, size_t n,
             uint64_t* out, uint32_t* flags) {
  const bool pt = op >= B2F_COP_FIELD_END;
  if (pt && (!za || !zb)) return B2F_ERR_ARG;
  const size_t el = pt ? 8 : 4;  // limbs per operand
  for (size_t i = 0; i < n * (el / 4); i++)
    if (!below_p<F>(a + 4 * i) || !below_p<F>(b + 4 * i)) return B2F_ERR_ARG;
  if (pt)
    for (size_t i = 0; i < n; i++)
      if (!below_p<F>(za + 4 * i) || !below_p<F>(zb + 4 * i)) return B2F_ERR_ARG;
  // a | b | za | zb | out | flags
  const size_t op_bytes = 8 * el * n, z_bytes = 32 * n;
  char* d = nullptr;
  if (hipMalloc(&d, 3 * op_bytes + 2 * z_bytes + 4 * n) != hipSuccess) return B2F_ERR_HIP;
  uint64_t* da = reinterpret_cast<uint64_t*>(d);
  uint64_t* db = reinterpret_cast<uint64_t*>(d + op_bytes);
  uint64_t* dza = reinterpret_cast<uint64_t*>(d + 2 * op_bytes);
  uint64_t* dzb = reinterpret_cast<uint64_t*>(d + 2 * op_bytes + z_bytes);
  uint64_t* dout = reinterpret_cast<uint64_t*>(d + 2 * op_bytes + 2 * z_bytes);
  uint32_t* dflags = reinterpret_cast<uint32_t*>(d + 3 * op_bytes + 2 * z_bytes);
  int rc = B2F_OK;
  if (hipMemset(d, 0, 3 * op_bytes + 2 * z_bytes + 4 * n) != hipSuccess ||
      hipMemcpy(da, a, op_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(db, b, op_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      (pt && (hipMemcpy(dza, za, z_bytes, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(dzb, zb, z_bytes, hipMemcpyHostToDevice) != hipSuccess)))
    rc = B2F_ERR_HIP;
  if (rc == B2F_OK) {
    hipLaunchKernelGGL(curve_op_kernel<F>, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, 0, da, db, dza, dzb,
                       (uint32_t)n, op, dout, dflags);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out, dout, op_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(flags, dflags, 4 * n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = B2F_ERR_HIP;
  }
  (void)hipFree(d);
  return rc;
}

}  // namespace
}  // namespace b2f

extern "C" B2F_API int b2f_debug_curve_op(uint32_t curve, uint32_t op, const uint64_t* a, const uint64_t* b,
                                          const uint64_t* za, const uint64_t* zb, size_t n, uint64_t* out,
                                          uint32_t* flags) {
  if (!a || !b || !out || !flags || n == 0 || n > 65536 || curve > 1 || op >= b2f::B2F_COP_COUNT)
    return B2F_ERR_ARG;
  return curve ? b2f::curve_op<b2f::field::Bn254Base>(op, a, b, za, zb, n, out, flags)
               : b2f::curve_op<b2f::field::VestaBase>(op, a, b, za, zb, n, out, flags);
}
