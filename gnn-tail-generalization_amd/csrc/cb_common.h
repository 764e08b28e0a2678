// Shared helpers for libcoldbrew_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/coldbrew_hip.h"

namespace cb {

constexpr int kWave = 64;  // CDNA wavefront

void set_error(const char* fmt, ...);
int* device_error_word();            // cb_error.hip: four ints of device-visible host memory (null if the allocation failed)
const char* device_error_text();     // what the word currently says

#define CB_CHECK_ARG(cond, code, ...)  \
  do {                                 \
    if (!(cond)) {                     \
      cb::set_error(__VA_ARGS__);      \
      return (code);                   \
    }                                  \
  } while (0)

#define CB_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      cb::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return CB_E_HIP;                                                                      \
    }                                                                                       \
  } while (0)

#define CB_LAUNCH_CHECK() CB_HIP(hipGetLastError())

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

static inline int blocks_for(int64_t n, int per_block) { return (int)((n + per_block - 1) / per_block); }

// the library's one alignment predicate: float4 / dwordx4 accesses need it of every row start
static inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// sum over the 64 lanes of a wavefront, every lane gets it: a fixed-order butterfly (deterministic)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// a*x + b*y and x*s + b with ONE fixed rounding sequence wherever they occur (residual mix: cb_axpby_f32 and the fused aggregation
// store; aggregation epilogue: plain and fused store).  Left to the compiler's contraction choice, the fused and the operator-by-
// operator forward differ in the last bit from one build to the next and the paths stop being bit-identical to each other.
__device__ __forceinline__ float mix2(float a, float x, float b, float y) { return __fmaf_rn(a, x, __fmul_rn(b, y)); }
__device__ __forceinline__ float scale_add(float x, float s, float b) { return __fmaf_rn(x, s, b); }

// The library's one ReLU.  fmaxf(v, 0.f) compiles to v_max_f32, which in IEEE mode returns the operand that is NOT a NaN: ReLU(NaN) came out 0, and the
// NaN the HIP path relies on as its loud failure signal (unread rows, bad pair endpoints, a diverged run) left every fused ReLU as a plausible zero.
// This form returns fmaxf(v, 0.f)'s bits for every v that is not a NaN (+0.0 for -0.0 and for every negative, subnormal or not; v itself above zero) and
// v itself for a NaN, as torch.relu and the oracle do.  One compare and one select in place of two maxima: profiles/relu_nan.md;
// tests/test_gpu_nonfinite.py holds every epilogue to it.  fmaxf stays where it is a maximum (running maxima, clamps).
__device__ __forceinline__ float relu_nan(float v) { return v <= 0.f ? 0.f : v; }

// wave-uniform broadcast helpers (values land in SGPRs)
__device__ __forceinline__ int bcast_first(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int bcast_lane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// bf16 storage helpers: the hardware's conversion (the one the three-limb split of cb_limb_core.h uses), two values per instruction.  Round to nearest,
// ties to even: torch's float -> bfloat16 conversion bit for bit on every input that is not a NaN — subnormals, carries into the exponent and the round-up
// to infinity included — and a NaN stays a NaN.  (The integer formula  u += 0x7FFF + ((u >> 16) & 1); u >> 16  that stood here is the same function off
// NaN, but its sum carries a NaN whose upper half is an infinity's, or all ones, into an infinity or a zero; with a NaN test in front of it the GEMM's and
// the layer backward's stores measured 3 % slower, with the conversion instruction 0.7 - 2 % faster: profiles/bf16_rounding.md.)
// tests/bf16_ref.py restates the conversion on the host; tests/test_gpu_bf16_storage.py holds every kernel that stores bf16 to it at the rounding edges.
typedef uint16_t bf16_t;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t cvt_pk_bf16(float x0, float x1) {   // {bf16(x0), bf16(x1)} in one dword (v_cvt_pk_bf16_f32)
  const f32x2 v = {x0, x1};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ bf16_t f32_to_bf16(float f) { return (bf16_t)(cvt_pk_bf16(f, 0.f) & 0xFFFFu); }
__device__ __forceinline__ float bf16_to_f32(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ uint2 pack4_bf16(float a, float b, float c, float d) { return make_uint2(cvt_pk_bf16(a, b), cvt_pk_bf16(c, d)); }

}  // namespace cb
