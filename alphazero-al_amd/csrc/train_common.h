// train_common.h - what the learner's four network pieces (train_block_kernels.hip, train_attn_kernels.hip,
// train_stem_kernels.hip, train_heads_kernels.hip) share: how a backward splits its samples into partial rows and what
// those rows take, the forward grid, and the few device functions at least two of them mean identically.
//
// Everything here is __device__ __forceinline__ or a host-side inline, in an anonymous namespace: a translation unit that
// includes it gets its own copy, no device code crosses translation units.  The rule is nn_common.h's: a helper belongs
// here only if every user means the same instructions by it.  What looks alike but adds in another order stays in its
// file under its own name (train_block_kernels.hip's block_sum, train_heads_kernels.hip's butterfly_sum).  The row-ordered
// sum at the head of each k_*_reduce stays in its kernel for the same reason: as an inlined function its loop compiles to
// another compare and branch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// ---- host: the backward's partition.  `rows` workgroups walk `per` contiguous samples each (the last one what is left)
// and leave one partial row each in the caller's workspace; max_workgroups 0 asks for the default cap.
constexpr int DEFAULT_ROWS = 256, MAX_ROWS = 1024;

struct Runs {
    int64_t per;
    int rows;
};

inline Runs partition(int64_t N, int max_workgroups)
{
    const int64_t cap = max_workgroups == 0 ? DEFAULT_ROWS : max_workgroups < MAX_ROWS ? max_workgroups : MAX_ROWS;
    const int64_t groups = N < cap ? N : cap;
    const int64_t per = (N + groups - 1) / groups;
    return Runs{per, static_cast<int>((N + per - 1) / per)};
}

// the batch sizes every entry point takes: sample offsets of n * 2688 floats stay far inside 64 bits, rows inside an int
inline bool n_ok(int64_t N) { return N > 0 && N <= (int64_t(1) << 30); }

inline int64_t rows_bytes(int64_t rows, int row_floats) { return rows * row_floats * static_cast<int64_t>(sizeof(float)); }

// the forward's workgroups: one per sample up to `cap`, beyond that a workgroup strides over the batch
inline unsigned fwd_grid(int64_t N, int cap) { return static_cast<unsigned>(N < cap ? N : cap); }

// ---- device
using f4 = float __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x4_f32: a k-ordered chain of float32 fused multiply-adds
__device__ __forceinline__ f4 mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ float sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }
// d/dz of z * sigmoid(z)
__device__ __forceinline__ float dsilu(float z) { const float s = sigmoid(z); return s + z * s * (1.0f - s); }

// the Connect4 board, and a plane of it in LDS with its ring of zeros (8 x 9): a tap outside the board reads a zero and a
// row cannot wrap
constexpr int ROWS = 6, COLS = 7;
constexpr int PW = COLS + 2, PAD = (ROWS + 2) * PW;
__device__ __forceinline__ int ring_pos(int cell) { return (cell / COLS + 1) * PW + cell % COLS + 1; }

}  // namespace
