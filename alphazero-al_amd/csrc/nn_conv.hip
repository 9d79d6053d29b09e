// nn_conv.hip - one residual convolution block of the evaluator as ONE MFMA kernel.
//
//   y = [x +] silu( conv3x3( [GroupNorm1(x) * gamma + beta] ) + bias )          (Network.py:27-48,166-170)
//
// on token-layout activations (B, 42, C) bf16.  The reference runs this as GroupNorm ->
// convolution -> (bias) -> SiLU -> add: four kernels and five passes over a 176 MB tensor per
// block at 32768 leaves.  Here a 4-wave workgroup owns a tile of 4 samples (168 tokens = 10.5
// MFMA tiles of 16), keeps their normalised, zero-padded 8x9 images in LDS and computes the
// 3x3 convolution as an implicit GEMM with v_mfma_f32_16x16x32_bf16 in the orientation
//
//   out^T (64 channels x tokens) = W (64 x 9*C_in) . X^T (9*C_in x tokens)
//
//   A operand = weights: wave (mh, th) owns output channels 32*mh.. and keeps its 2 x (K/32)
//               fragments in registers (144 VGPRs at C_in = 64) for the whole kernel;
//   B operand = one ds_read_b128 per lane: 8 input channels of the tap's neighbour cell of
//               token (lane & 15).  Cells are 128 B; the 16-byte chunk index is XORed with
//               (cell & 7), which makes every read group of 16 consecutive cells hit 16
//               distinct bank slots (cdna guide T2) - the padded-stride layout this replaces
//               was 2-way conflicted on every read;
//   C layout  = 4 consecutive output channels of one token per lane: bias + SiLU + residual
//               happen on the accumulators and leave as 8-byte stores, no staging pass.
//
// Two token tiles share each weight fragment (4 MFMAs per 2 LDS reads).  79 KB of LDS (C_in 64 with
// the residual: 80 896 B - 36 864 for the images, 43 008 for two raw tiles, 1 024 for gamma / beta
// and the dummy slots; k_stem_conv_block: 80 640 B with ONE raw tile and the stem's two tables) and
// <= 256 VGPRs let two workgroups share a CU, so one workgroup's load / GroupNorm / epilogue
// VALU work overlaps the other's MFMA phase; workgroups are persistent over tiles and fetch
// the next tile's activations while the current one is multiplied.  HBM traffic per block:
// read x once, write y once (the residual is re-read from an LDS copy of the raw tile).
//
// k_stem_conv_block is the first residual block with the folded stem (nn_stem.hip) computed in front of
// it: no x is read at all, each wavefront builds the raw tile of its sample from the leaf's position.
//
// k_conv_chain is that kernel and the residual blocks behind it in ONE launch: the body once per layer, the activations
// through HBM / L2 between layers exactly as between the separate launches, no grid-wide barrier (layer_switch below).
#include <cstdio>
#include <cstdlib>

#include "az_nn.h"
#include "nn_common.h"

namespace {

constexpr int CELLS = 42, COLS = 7;
// Zero-padded image with a row pitch of 8 cells: the right halo of a row IS the left halo of the
// next one (both zero), so cell p = (r+1)*8 + (c+1) and p & 7 - the swizzle key - depends on the
// column only: the three rows of a 3x3 window are the same address +- 1 KiB.
constexpr int PCOLS = 8, PCELLS = 72;          // 65 cells used
constexpr int TS = 4;                          // samples per tile = wavefronts per workgroup
constexpr int COUT = 64;
constexpr int CELLB = 128;                     // bytes per image cell (C_in 32 uses half of it)

// A sample's raw vectors from global memory straight into LDS, 16 bytes per lane and instruction, as ONE statement:
// vector i of lane l comes from base + voff(l) + 1024 i and lands at lds_off + 1024 i + 16 l (the LDS side of the
// instruction is wave-uniform base + lane order); N = 6 vectors (64 channels) or 3 (32), the last one in the lanes of
// last_mask only.  Inline assembly on purpose: when the compiler knows that a global_load_lds is in flight it puts
// s_waitcnt vmcnt(0) in front of every later LDS read that might alias it, i.e. at the top of the MFMA phase, and the
// HBM latency this staging is meant to hide is paid in full.  The kernel orders the accesses itself (vmcnt(0) + barrier
// before the buffer is read).
// base is wave-uniform (an SGPR pair) and 1024 i sits in the instruction's offset field, which is added to the global
// address AND to the LDS address (the compiler's own __builtin_amdgcn_global_load_lds(g, l, 16, 1024, 0) sets M0 to l
// and the field to 1024), so M0 is written once per group of four (the field is 13-bit signed: up to 3072).  M0 is
// compiler-reserved: saved and restored inside the statement, once.  The s_nop cover an SGPR base written by a VALU
// (5 states) and the M0 write (1).
template <int N>
__device__ __forceinline__ void stage_sample(const void *base, uint32_t voff, uint32_t lds_off, uint64_t last_mask)
{
    uint32_t keep;
    uint64_t ex;
    if constexpr (N == 6)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 2\n\t"
                     "global_load_lds_dwordx4 %2, %3\n\t"
                     "global_load_lds_dwordx4 %2, %3 offset:1024\n\t"
                     "global_load_lds_dwordx4 %2, %3 offset:2048\n\t"
                     "global_load_lds_dwordx4 %2, %3 offset:3072\n\t"
                     "s_mov_b32 m0, %6\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %5, %3\n\t"
                     "s_and_saveexec_b64 %1, %7\n\t"
                     "global_load_lds_dwordx4 %5, %3 offset:1024\n\t"
                     "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep), "=&s"(ex)
                     : "v"(voff), "s"(base), "s"(lds_off), "v"(voff + 4096), "s"(lds_off + 4096), "s"(last_mask)
                     : "memory", "scc");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 2\n\t"
                     "global_load_lds_dwordx4 %2, %3\n\t"
                     "global_load_lds_dwordx4 %2, %3 offset:1024\n\t"
                     "s_and_saveexec_b64 %1, %5\n\t"
                     "global_load_lds_dwordx4 %2, %3 offset:2048\n\t"
                     "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep), "=&s"(ex)
                     : "v"(voff), "s"(base), "s"(lds_off), "s"(last_mask)
                     : "memory", "scc");
}
__device__ __forceinline__ uint32_t lds_addr(const void *p)
{
    return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) const void *)p));
}
// workgroup barrier that orders LDS traffic only: __syncthreads() would also wait for this
// wave's outstanding global stores
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// az_nn_debug bit 4: per-wave cycle totals of the phases (s_memtime), read back by az_nn_conv_profile
__device__ unsigned long long g_prof[2048 * 8];

// what the stem needs to build its input tokens itself (EMBED): the evaluator's feature planes and
// the embedding tables of Network.py:226-239
struct EmbedIn {
    const float    *features;          // (rows, 3, 6, 7) relative planes
    const uint16_t *emb_own, *emb_opp; // (32,) bf16
    const uint16_t *pos;               // (42, 32) bf16
    const int32_t  *gather;            // compact sample b shows row gather[b] (NULL: b)
    // features == nullptr: the planes are built from the leaf POSITIONS instead (no feature tensor in HBM):
    // two bitboards (bit = 7 * column + height, Connect4.h:15-29), side to move, symmetry id (1 = mirrored)
    const uint64_t *bb_p1, *bb_p2;
    const int32_t  *turn, *sym;
};

// what the first residual block needs to compute the folded stem of its tile itself (STEM, nn_stem.hip's arithmetic):
// the leaf positions and the two tables of fast_net.fold_stem
struct StemIn {
    const uint64_t *bb_p1, *bb_p2;     // as EmbedIn
    const int32_t  *turn, *sym;
    const int32_t  *gather;            // compact sample b shows row gather[b] (NULL: b)
    const uint16_t *wfrag;             // bf16 [2][4][64][8]: the table's high and low part in fragment order
    const float    *pmap;              // float32 [48][68]
};
constexpr int PROWS = 48, PROW = 68;           // pmap: 48 token rows (42 used, the rest zero) of 68 floats (64 used)
constexpr int PMAPB = PROWS * PROW * 4, FRAGB = 2 * 4 * 64 * 16;

// The kernels of this file share one body, nn_conv_body.h, as TEXT: included, a kernel without STEM compiles to the
// instruction stream it had before STEM existed; called as a __forceinline__ template the same text was scheduled
// differently.
template <int CIN, bool NORM, bool RESID, bool EMBED = false>
__global__ void __launch_bounds__(256, 2) k_conv_block(const uint16_t *x, const uint16_t *w, const uint16_t *bias,
                                                       const uint16_t *gamma, const uint16_t *beta, uint16_t *y,
                                                       int64_t B, float eps, int dbg, const int64_t *batch_dev, EmbedIn em)
{
    constexpr bool STEM = false, CHAINED = false;
    const StemIn st{};
#include "nn_conv_body.h"
}

// the folded stem and the first residual block (C_in 64, normalised, residual) as one launch
__global__ void __launch_bounds__(256, 2) k_stem_conv_block(StemIn st, const uint16_t *w, const uint16_t *bias,
                                                            const uint16_t *gamma, const uint16_t *beta, uint16_t *y,
                                                            int64_t B, float eps, int dbg, const int64_t *batch_dev)
{
    constexpr int CIN = 64;
    constexpr bool NORM = true, RESID = true, EMBED = false, STEM = true, CHAINED = false;
    const uint16_t *x = nullptr;
    const EmbedIn em{};
#include "nn_conv_body.h"
}

// k_conv_chain: the folded stem with the first residual block and the residual blocks behind it, layer after layer in
// ONE launch.  Per-layer arguments, by value: layer L reads y[L - 1] (layer 0: the positions) and writes y[L].
struct ChainIn {
    const uint16_t *w[AZ_NN_MAX_BLOCKS], *bias[AZ_NN_MAX_BLOCKS], *gamma[AZ_NN_MAX_BLOCKS], *beta[AZ_NN_MAX_BLOCKS];
    uint16_t *y[AZ_NN_MAX_BLOCKS];
    int n;
};

// Between two layers of k_conv_chain.  The launches this kernel replaces use the same grid, the same tile order (tile =
// blockIdx.x + k * gridDim.x) and the same wave-to-sample rule (wave s stages and stores sample tile * 4 + s), so the only
// reader of what a wave stored in layer L is that same wave in layer L + 1: no workgroup waits for another one.  The wave
// waits for its own stores - the L1 is write-through: they are then in the L2 of this CU's XCD, the one its loads are
// served from - and an agent-scope ACQUIRE drops the lines its CU's L1 may still hold of the buffer it reads next (layer
// L + 1 writes the buffer layer L read - the two scratch tensors ping-pong - so a line cached two layers ago would be
// stale).  No release: nothing outside this CU reads the activations before the kernel ends, and the write-back of the
// whole L2 that an agent-scope release (__threadfence()) performs made the kernel 97 us slower than the launches it
// replaces (EXPERIMENTS.md E21).  The barrier keeps the next prologue's LDS zeroing behind every wave's last reads of
// the output tile.
__device__ __forceinline__ void layer_switch()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __syncthreads();
}

// The body once with the stem in front (layer 0) and once more, in a loop that is not unrolled, for the layers behind
// it: the same text as the kernels above, so every layer computes the bytes its own launch would have.  The first
// inclusion clamps B from batch_dev; the others find it clamped (their batch_dev is null) and restart at raw buffer 0
// (par is the body's own).  Dynamic LDS: the larger of the two layouts.
__global__ void __launch_bounds__(256, 2) k_conv_chain(StemIn st_in, ChainIn ch, int64_t B, float eps, int dbg, const int64_t *batch_dev_in)
{
    constexpr int CIN = 64;
    constexpr bool NORM = true, RESID = true, EMBED = false;
    const EmbedIn em{};
    {
        constexpr bool STEM = true, CHAINED = false;
        const StemIn &st = st_in;
        const uint16_t *x = nullptr, *w = ch.w[0], *bias = ch.bias[0], *gamma = ch.gamma[0], *beta = ch.beta[0];
        uint16_t *y = ch.y[0];
        const int64_t *batch_dev = batch_dev_in;
#include "nn_conv_body.h"
    }
#pragma unroll 1
    for (int layer = 1; layer < ch.n; ++layer) {
        layer_switch();
        constexpr bool STEM = false, CHAINED = true;
        const StemIn st{};
        const uint16_t *x = ch.y[layer - 1], *w = ch.w[layer], *bias = ch.bias[layer], *gamma = ch.gamma[layer], *beta = ch.beta[layer];
        uint16_t *y = ch.y[layer];
        const int64_t *batch_dev = nullptr;
#include "nn_conv_body.h"
    }
}

// az_nn_debug: timing experiments (1 skips the MFMA loop, 2 skips the store, ...: bits 0-7 go to the kernels of this file)
// and the grid cap of nn_attn_heads.hip (az_nn_debug_flags)
int g_dbg = 0;

// What a launch of either kernel does once its pointer and its dynamic LDS bytes are known: the once-per-device set-up
// (with AZ_NN_VERBOSE: the occupancy line; c_in 0 words it for k_stem_conv_block, c_in < 0 for k_conv_chain), then the grid - one workgroup per
// tile of TS samples, at most AZ_NN_CONV_GRID - and the kernel's dbg word.  `setup` is the caller's: one static
// DeviceSetup per kernel instantiation (nn_common.h).  The environment is read once per process.  Returns 0, or 2 when
// the device refused the set-up.
int prepare(DeviceSetup &setup, const void *kern, size_t smem, int c_in, int64_t B, unsigned &grid, int &dbg)
{
    if (setup.cus({kern}, static_cast<int>(smem), [&] {
            if (getenv("AZ_NN_VERBOSE") != nullptr) {
                int per_cu = 0;
                (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, smem);
                if (c_in < 0)
                    fprintf(stderr, "[az_nn] stem + conv chain: %zu B LDS, %d workgroups per CU\n", smem, per_cu);
                else if (c_in != 0)
                    fprintf(stderr, "[az_nn] conv block C_in=%d: %zu B LDS, %d workgroups per CU\n", c_in, smem, per_cu);
                else
                    fprintf(stderr, "[az_nn] stem + conv block: %zu B LDS, %d workgroups per CU\n", smem, per_cu);
            }
        }) == 0)
        return 2;
    // issue priority of the matrix phase over the other workgroup's load / store phases (s_setprio 0..3; AZ_NN_CONV_PRIO)
    static const int prio = [] { const char *e = getenv("AZ_NN_CONV_PRIO"); const int v = e ? atoi(e) : 1; return v < 0 || v > 3 ? 1 : v; }();
    const int64_t ntiles = (B + TS - 1) / TS;
    static const int64_t max_grid = getenv("AZ_NN_CONV_GRID") ? atoll(getenv("AZ_NN_CONV_GRID")) : 512;   // two workgroups per CU
    grid = static_cast<unsigned>(ntiles < max_grid ? ntiles : max_grid);
    dbg = (g_dbg & 255) | (((g_dbg >> 5) & 3) ? 0 : (prio << 5));
    return 0;
}

template <int CIN, bool NORM, bool RESID, bool EMBED = false>
int launch(const void *x, const void *w, const void *bias, const void *gamma, const void *beta, void *y, int64_t B,
           float eps, const int64_t *batch_dev, hipStream_t s, EmbedIn em = EmbedIn{})
{
    constexpr size_t smem = static_cast<size_t>(TS) * PCELLS * CELLB + 2 * static_cast<size_t>(TS) * CELLS * CIN * 2 +
                            (RESID ? 0 : static_cast<size_t>(TS) * CELLS * COUT * 2) + 2 * CIN * sizeof(float) + 512;
    auto kern = k_conv_block<CIN, NORM, RESID, EMBED>;
    static DeviceSetup setup;
    unsigned grid;
    int dbg;
    if (prepare(setup, reinterpret_cast<const void *>(kern), smem, CIN, B, grid, dbg) != 0) return 2;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, s, static_cast<const uint16_t *>(x),
                       static_cast<const uint16_t *>(w), static_cast<const uint16_t *>(bias),
                       static_cast<const uint16_t *>(gamma), static_cast<const uint16_t *>(beta),
                       static_cast<uint16_t *>(y), B, eps, dbg, batch_dev, em);
    return 0;
}

int launch_stem(const StemIn &st, const void *w, const void *bias, const void *gamma, const void *beta, void *y, int64_t B,
                float eps, const int64_t *batch_dev, hipStream_t s)
{
    // images, ONE raw tile, gamma / beta + the dummy slots, the stem's two tables
    constexpr size_t smem = static_cast<size_t>(TS) * PCELLS * CELLB + static_cast<size_t>(TS) * CELLS * 64 * 2 +
                            2 * 64 * sizeof(float) + 512 + PMAPB + FRAGB;
    static_assert(2 * smem <= 160 * 1024, "two workgroups per CU");
    static DeviceSetup setup;
    unsigned grid;
    int dbg;
    if (prepare(setup, reinterpret_cast<const void *>(k_stem_conv_block), smem, 0, B, grid, dbg) != 0) return 2;
    hipLaunchKernelGGL(k_stem_conv_block, dim3(grid), dim3(256), smem, s, st, static_cast<const uint16_t *>(w),
                       static_cast<const uint16_t *>(bias), static_cast<const uint16_t *>(gamma),
                       static_cast<const uint16_t *>(beta), static_cast<uint16_t *>(y), B, eps, dbg, batch_dev);
    return 0;
}

int launch_chain(const StemIn &st, const ChainIn &ch, int64_t B, float eps, const int64_t *batch_dev, hipStream_t s)
{
    // the larger of the two layouts: the blocks' (images, TWO raw tiles, gamma / beta + the dummy slots) and the stem
    // block's (launch_stem)
    constexpr size_t smem_block = static_cast<size_t>(TS) * PCELLS * CELLB + 2 * static_cast<size_t>(TS) * CELLS * 64 * 2 +
                                  2 * 64 * sizeof(float) + 512;
    constexpr size_t smem_stem = static_cast<size_t>(TS) * PCELLS * CELLB + static_cast<size_t>(TS) * CELLS * 64 * 2 +
                                 2 * 64 * sizeof(float) + 512 + PMAPB + FRAGB;
    constexpr size_t smem = smem_block > smem_stem ? smem_block : smem_stem;
    static_assert(smem == 80896 && 2 * smem <= 160 * 1024, "two workgroups per CU");
    static DeviceSetup setup;
    unsigned grid;
    int dbg;
    if (prepare(setup, reinterpret_cast<const void *>(k_conv_chain), smem, -1, B, grid, dbg) != 0) return 2;
    hipLaunchKernelGGL(k_conv_chain, dim3(grid), dim3(256), smem, s, st, ch, B, eps, dbg, batch_dev);
    return 0;
}

}  // namespace

extern "C" {

int az_nn_debug(int flags) { g_dbg = flags; return 0; }
int az_nn_debug_flags(void) { return g_dbg; }

int az_nn_conv_profile(unsigned long long *out, int n)
{
    if (n > 2048 * 8) n = 2048 * 8;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * n) == hipSuccess ? 0 : 2;
}

int az_nn_conv_block(const void *x, int c_in, const void *weight_ohwi, const void *bias, const void *gamma,
                     const void *beta, int residual, void *y, int64_t batch, float eps, const int64_t *batch_dev,
                     void *stream)
{
    if (batch <= 0) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool norm = gamma != nullptr && beta != nullptr;
    if (c_in == 64 && norm && residual) return launch<64, true, true>(x, weight_ohwi, bias, gamma, beta, y, batch, eps, batch_dev, s);
    if (c_in == 64 && norm && !residual) return launch<64, true, false>(x, weight_ohwi, bias, gamma, beta, y, batch, eps, batch_dev, s);
    if (c_in == 32 && !norm && !residual) return launch<32, false, false>(x, weight_ohwi, bias, gamma, beta, y, batch, eps, batch_dev, s);
    return 1;
}

int az_nn_stem_conv_block_positions(const az_nn_positions *positions, const void *w_frag, const float *pmap,
                                    const void *weight_ohwi, const void *bias, const void *gamma, const void *beta, void *y,
                                    int64_t batch, float eps, const int32_t *gather, const int64_t *batch_dev, void *stream)
{
    if (batch <= 0 || positions == nullptr || !positions->bb_p1 || !positions->bb_p2 || !positions->turn || !positions->sym ||
        w_frag == nullptr || pmap == nullptr || weight_ohwi == nullptr || bias == nullptr || gamma == nullptr || beta == nullptr ||
        y == nullptr)
        return 1;
    const StemIn st{positions->bb_p1, positions->bb_p2, positions->turn, positions->sym, gather,
                    static_cast<const uint16_t *>(w_frag), pmap};
    return launch_stem(st, weight_ohwi, bias, gamma, beta, y, batch, eps, batch_dev, static_cast<hipStream_t>(stream));
}

int az_nn_stem_conv_chain_positions(const az_nn_positions *positions, const void *w_frag, const float *pmap, int n_blocks,
                                    const void *const *weight_ohwi, const void *const *bias, const void *const *gamma,
                                    const void *const *beta, void *y_even, void *y_odd, int64_t batch, float eps,
                                    const int32_t *gather, const int64_t *batch_dev, void *stream)
{
    if (batch <= 0 || positions == nullptr || !positions->bb_p1 || !positions->bb_p2 || !positions->turn || !positions->sym ||
        w_frag == nullptr || pmap == nullptr || n_blocks < 1 || n_blocks > AZ_NN_MAX_BLOCKS || weight_ohwi == nullptr ||
        bias == nullptr || gamma == nullptr || beta == nullptr || y_even == nullptr || y_odd == nullptr || y_even == y_odd)
        return 1;
    ChainIn ch{};
    for (int i = 0; i < n_blocks; ++i) {
        if (!weight_ohwi[i] || !bias[i] || !gamma[i] || !beta[i]) return 1;
        ch.w[i] = static_cast<const uint16_t *>(weight_ohwi[i]);
        ch.bias[i] = static_cast<const uint16_t *>(bias[i]);
        ch.gamma[i] = static_cast<const uint16_t *>(gamma[i]);
        ch.beta[i] = static_cast<const uint16_t *>(beta[i]);
        ch.y[i] = static_cast<uint16_t *>((i & 1) ? y_odd : y_even);
    }
    ch.n = n_blocks;
    const StemIn st{positions->bb_p1, positions->bb_p2, positions->turn, positions->sym, gather,
                    static_cast<const uint16_t *>(w_frag), pmap};
    return launch_chain(st, ch, batch, eps, batch_dev, static_cast<hipStream_t>(stream));
}

int az_nn_stem_embed(const float *features, const void *emb_own, const void *emb_opp, const void *pos,
                     const void *weight_ohwi, const void *bias, void *y, int64_t batch, const int32_t *gather,
                     const int64_t *batch_dev, void *stream)
{
    if (batch <= 0 || features == nullptr) return 1;
    EmbedIn em{features, static_cast<const uint16_t *>(emb_own), static_cast<const uint16_t *>(emb_opp),
               static_cast<const uint16_t *>(pos), gather, nullptr, nullptr, nullptr, nullptr};
    return launch<32, false, false, true>(nullptr, weight_ohwi, bias, nullptr, nullptr, y, batch, 0.0f, batch_dev,
                                          static_cast<hipStream_t>(stream), em);
}

int az_nn_stem_embed_positions(const az_nn_positions *positions, const void *emb_own, const void *emb_opp, const void *pos,
                               const void *weight_ohwi, const void *bias, void *y, int64_t batch, const int32_t *gather,
                               const int64_t *batch_dev, void *stream)
{
    if (batch <= 0 || positions == nullptr || !positions->bb_p1 || !positions->bb_p2 || !positions->turn || !positions->sym) return 1;
    EmbedIn em{nullptr, static_cast<const uint16_t *>(emb_own), static_cast<const uint16_t *>(emb_opp),
               static_cast<const uint16_t *>(pos), gather, positions->bb_p1, positions->bb_p2, positions->turn, positions->sym};
    return launch<32, false, false, true>(nullptr, weight_ohwi, bias, nullptr, nullptr, y, batch, 0.0f, batch_dev,
                                          static_cast<hipStream_t>(stream), em);
}

}  // extern "C"
