// quant_math.h — the per-element arithmetic of QuantizedValue.quantize / to_float
// (precondition/quantization_utils.py:85-94 and :108-112, "QU"), shared by quant.hip and the int8-momentum
// kernels of transform.hip.  Every operation is one IEEE float32 rounding (the including object is built
// with -ffp-contract=off): codes and bucket sizes are the reference's bits on every path that uses these.
#pragma once
#include <hip/hip_runtime.h>

namespace psk {

// QU:56-63: the most negative code is never used
__device__ __forceinline__ float num_buckets(int bits) { return bits == 8 ? 127.f : 32767.f; }
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

// Four consecutive codes <-> one store: int16 as 8 bytes, int8 as 4 (code j at the lower address)
__device__ __forceinline__ uint2 pack4_i16(const int (&q)[4]) {
  return uint2{((unsigned)q[0] & 0xffffu) | ((unsigned)q[1] << 16), ((unsigned)q[2] & 0xffffu) | ((unsigned)q[3] << 16)};
}
__device__ __forceinline__ unsigned pack4_i8(const int (&q)[4]) {
  return ((unsigned)q[0] & 0xffu) | (((unsigned)q[1] & 0xffu) << 8) | (((unsigned)q[2] & 0xffu) << 16) |
         ((unsigned)q[3] << 24);
}
__device__ __forceinline__ void unpack4_i16(uint2 pk, int (&q)[4]) {
  q[0] = (short)(pk.x & 0xffffu); q[1] = (short)(pk.x >> 16);
  q[2] = (short)(pk.y & 0xffffu); q[3] = (short)(pk.y >> 16);
}
__device__ __forceinline__ void unpack4_i8(unsigned pk, int (&q)[4]) {
  q[0] = (signed char)(pk & 0xffu); q[1] = (signed char)((pk >> 8) & 0xffu);
  q[2] = (signed char)((pk >> 16) & 0xffu); q[3] = (signed char)(pk >> 24);
}

}  // namespace psk
