// nn_common.h - what the evaluator's kernel files share: vector types, bf16 packing, the fast transcendental forms,
// reductions inside a wavefront, the MFMA shorthands, and the once-per-device setup of a host entry point.
//
// Everything here is __device__ __forceinline__ in an anonymous namespace (or a host-side inline): a translation unit
// that includes it gets its own copy, no device code crosses translation units.  A helper belongs here only if every
// user means the same instructions by it; variants (nn_kernels.hip's pack_bf16, nn_othello.hip's round_bf) stay in their files under their own names.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <mutex>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
struct alignas(16) V8 { uint32_t w[4]; };      // 8 bf16: one 16-byte load / store, one 16x16x32 MFMA operand
struct alignas(8) V4 { uint32_t w[2]; };       // 4 bf16: one 16x16x16 MFMA operand

// ---- bf16 <-> f32
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ float bf1(const uint16_t *p) { return __uint_as_float(static_cast<uint32_t>(*p) << 16); }
// one v_cvt_pk_bf16_f32 (round to nearest even, NaN preserving)
__device__ __forceinline__ uint32_t pack2(float a, float b)
{
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
// packed-f32 arithmetic (v_pk_mul/add/fma_f32): two elements per VALU instruction
__device__ __forceinline__ f32x2 unpack2(uint32_t w) { return f32x2{bf_lo(w), bf_hi(w)}; }
__device__ __forceinline__ f32x2 rbf2(f32x2 v) { return unpack2(pack2(v.x, v.y)); }       // round to bf16 and back
__device__ __forceinline__ s16x4 to_s16x4(const f32x4 &v)
{
    union { uint32_t u[2]; s16x4 s; } r;
    r.u[0] = pack2(v[0], v[1]);
    r.u[1] = pack2(v[2], v[3]);
    return r.s;
}
__device__ __forceinline__ bf16x8 as_bf16x8(const V8 &v)
{
    union { V8 a; bf16x8 b; } r;
    r.a = v;
    return r.b;
}

// ---- silu / exp with the hardware exp2 and reciprocal (about 1 ulp each; the results are rounded to bf16)
__device__ __forceinline__ f32x2 silu2(f32x2 x)
{
    const f32x2 t = x * f32x2{-1.44269504f, -1.44269504f};
    const f32x2 e = f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)} + f32x2{1.0f, 1.0f};
    return x * f32x2{__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
}
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(1.44269504f * x); }
// One v_rsq_f32.  PRECONDITION: x >= FLT_MIN (or NaN).  rsqrtf() wraps the instruction in a guard for the denormal range
// (scale by 2^24 below FLT_MIN, select, rescale: five more instructions); at and above FLT_MIN the guard picks the
// unscaled operand, so this returns rsqrtf()'s bits.  For the RMS statistics sum / n + eps that means eps >= FLT_MIN:
// the host entry points launch the rsqrtf() forms of their kernels for a smaller eps.
__device__ __forceinline__ float rsq_normal(float x) { return __builtin_amdgcn_rsqf(x); }

// ---- reductions inside a wavefront.  Along a 16-lane row: DPP, the lane movement is an operand modifier of the add
// (no LDS crossbar, no address arithmetic).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float sum8(float v)      // over the 8 lanes that share lane >> 3; result in all of them
{
    v += dpp_mov<0xB1>(v);           // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);           // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);          // row_half_mirror
    return v;
}
__device__ __forceinline__ float sum16(float v) { v = sum8(v); return v + dpp_mov<0x140>(v); }   // + row_mirror: the 16-lane row
// sum16() with every step kept a scalar add, so that the lane movement folds into it (v_add_f32_dpp).  A caller that
// builds a float pair from two sum16() results has its adds vectorised into v_pk_add_f32, which takes no DPP operand
// and so needs a v_mov_b32_dpp per step next to it; the empty statement hides each sum from the vectoriser and emits
// nothing.  The same additions in the same order as sum16().
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)
{
    v += dpp_mov<CTRL>(v);
    asm("" : "+v"(v));
    return v;
}
__device__ __forceinline__ float sum16_dpp(float v)
{
    return dpp_add<0x140>(dpp_add<0x141>(dpp_add<0x4E>(dpp_add<0xB1>(v))));
}
__device__ __forceinline__ float max8(float v)
{
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    return v;
}
// over the wavefront, returned uniform: 8 VALU instructions and a readlane, against 6 x (ds_bpermute + address + add)
__device__ __forceinline__ float wave_sum(float v)
{
    v = sum16(v);
    v += dpp_mov<0x142, 0xa>(v);     // row_bcast:15 into rows 1 and 3
    v += dpp_mov<0x143, 0xc>(v);     // row_bcast:31 into rows 2 and 3: lane 63 holds the total
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// Across the 4 lane groups that share lane & 15 (the rows of a column in the MFMA C layout) on the vector ALU:
// v_permlane16_swap / v_permlane32_swap (gfx950) hand every lane its partner across rows {0,1},{2,3} and across the
// wavefront's halves - two instructions per step where __shfl_xor takes a trip through the LDS crossbar
// (ds_bpermute + address + wait) each.
__device__ __forceinline__ float col_sum(float v)
{
    u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r.x) + __uint_as_float(r.y);
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ float col_max(float v)
{
    u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r.x), __uint_as_float(r.y));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r.x), __uint_as_float(r.y));
}
// Two independent values through ONE set of swaps: a = col_sum(a), b = col_sum(b), bit for bit (the same additions in
// the same grouping, (v0 + v1) + (v2 + v3) over the rows).  With rows written [r0, r1, r2, r3]:
//   permlane16_swap(a, b), add  -> [a0+a1, b0+b1, a2+a3, b2+b3]
//   permlane32_swap(t, t), add  -> [A, B, A, B]
//   permlane16_swap(u, u)       -> A in every row of one register, B in every row of the other
// 3 swaps, 2 adds and 2 copies where two col_sum() calls take 4, 4 and 4.
template <class Op>
__device__ __forceinline__ void col_reduce2(float &a, float &b, Op op)
{
    u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    const float t = op(__uint_as_float(r.x), __uint_as_float(r.y));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(t), __float_as_uint(t), false, false);
    const float u = op(__uint_as_float(r.x), __uint_as_float(r.y));
    r = __builtin_amdgcn_permlane16_swap(__float_as_uint(u), __float_as_uint(u), false, false);
    a = __uint_as_float(r.x);
    b = __uint_as_float(r.y);
}
__device__ __forceinline__ void col_sum2(float &a, float &b) { col_reduce2(a, b, [](float x, float y) { return x + y; }); }
__device__ __forceinline__ void col_max2(float &a, float &b) { col_reduce2(a, b, [](float x, float y) { return fmaxf(x, y); }); }
// LDS traffic between lanes of ONE wavefront: the LDS executes a wavefront's instructions in order, so only the
// compiler has to be stopped from moving accesses across this point.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k((a), (b), (c), 0, 0, 0)

// ---- host: what an entry point does once per DEVICE before its first launch there - raise the dynamic-LDS limit of
// its kernels (the attribute is per device) and fetch the CU count.  Engines are driven from several host threads, so
// the first calls may arrive together: std::call_once.  One `static DeviceSetup` per entry point (per instantiation of
// a templated launcher).
class DeviceSetup {
public:
    // CU count of the current device, or 0 if the device or one of the attributes was refused (the caller returns 2).
    // `first` runs once per device after a successful setup (a verbose report, say).
    template <class First>
    int cus(std::initializer_list<const void *> kernels, int lds_bytes, First first)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
        Slot &s = slot_[dev];
        std::call_once(s.once, [&] {
            for (const void *k : kernels)
                if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) return;
            int n = 0;
            if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return;
            s.cus = n;
            first();
        });
        return s.cus;
    }
    int cus(std::initializer_list<const void *> kernels, int lds_bytes) { return cus(kernels, lds_bytes, [] {}); }

private:
    static constexpr int kMaxDevices = 64;
    struct Slot {
        std::once_flag once;
        int cus = 0;
    } slot_[kMaxDevices];
};

}  // namespace
