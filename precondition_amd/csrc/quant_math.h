// quant_math.h — the per-element arithmetic of QuantizedValue.quantize / to_float
// (precondition/quantization_utils.py:85-94 and :108-112, "QU"), shared by quant.hip and the int8-momentum
// kernels of transform.hip.  Every operation is one IEEE float32 rounding (the including object is built
// with -ffp-contract=off): codes and bucket sizes are the reference's bits on every path that uses these.
#pragma once
#include <hip/hip_runtime.h>

namespace psk {

// QU:86 from the bit pattern of a column's max |x| (non-negative floats order like their bits)
__device__ __forceinline__ float bucket_size(unsigned colmax_bits, float num_buckets) {
  return __fdiv_rn(__uint_as_float(colmax_bits), num_buckets);
}
// QU:89-90
__device__ __forceinline__ float bucket_nonzero(float bs) { return bs > 0.f ? bs : 1.f; }
// QU:91-94; rint = round half to even
__device__ __forceinline__ int encode1(float x, float bs_nonzero) {
  return (int)rintf(__fdiv_rn(x, bs_nonzero));
}
// QU:109
__device__ __forceinline__ float decode1(int code, float bs) { return __fmul_rn((float)code, bs); }

}  // namespace psk
