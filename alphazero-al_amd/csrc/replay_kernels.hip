// replay_kernels.hip - the learner's data side: training batches straight out of the replay ring in HBM
// (az_replay_dev_batch and az_replay_dev_sample_indices in az_mcts.h).
//
//   k_replay_batch    B ring rows picked by index -> one ready-to-train batch of S * B rows: the gather
//                     (ReplayBuffer.py:125-128, `get`), the int8 -> float32 cast of the planes, and the game's
//                     symmetry augmentation (Connect4/utils.py:50-67: identity and the column mirror;
//                     Othello/utils.py:65-91: the reference's ids 0, 2, 6, 7) in one launch.  Output row s * B + b
//                     is sample b under symmetry s - what `augment(get(idx))` returns.  One wavefront per sample:
//                     it reads the source row once into registers (lane l keeps unit l of the state, action l of
//                     prob and mask), builds every symmetry's row with lane shuffles and writes each with
//                     consecutive lanes on consecutive addresses - 16-byte stores for Othello's 768-byte state
//                     rows, 8-byte stores for Connect4's 504-byte rows (63 x 8; not a multiple of 16).  No LDS,
//                     no atomics.  The symmetry maps are compile-time per game; all are involutions, so source
//                     cell and destination cell of a map are interchangeable.
//   k_replay_indices  n ring indices uniform in [0, n_valid) from the device generator (dev_rng.h), in place of the
//                     host's np.random.randint of ReplayBuffer.py:142.
//
// Plain C++ and vector stores only.
#include "kernels.h"

#include "dev_rng.h"
#include "games.h"

namespace az {
namespace {

constexpr int WAVE = 64;

template <class G> struct Augment;
template <> struct Augment<Connect4Dev> {
    static constexpr int S = 2;
    using SrcUnit = uint16_t;      // 126-byte source rows: consecutive rows are 2-byte aligned
    using OutUnit = float2;        // 504-byte output rows: 8-byte aligned
    // the cell that symmetry s pairs with `cell`: identity, c -> 6 - c
    __device__ static constexpr int cell(int s, int cell)
    {
        return s == 0 ? cell : (cell / 7) * 7 + 6 - cell % 7;
    }
    __device__ static constexpr int action(int s, int a) { return s == 0 ? a : 6 - a; }
};
template <> struct Augment<OthelloDev> {
    static constexpr int S = 4;
    using SrcUnit = uint32_t;      // 192-byte source rows
    using OutUnit = float4;        // 768-byte output rows: 16-byte aligned
    // identity, (r, c) -> (7 - r, 7 - c), (r, c) -> (c, r), (r, c) -> (7 - c, 7 - r)
    __device__ static constexpr int cell(int s, int cell)
    {
        const int r = cell / 8, c = cell % 8;
        return s == 0 ? cell : s == 1 ? 63 - cell : s == 2 ? c * 8 + r : (7 - c) * 8 + 7 - r;
    }
    __device__ static constexpr int action(int s, int a) { return a < 64 ? cell(s, a) : a; }   // the pass stays
};

__device__ __forceinline__ void put(float2 &v, int j, float x) { if (j == 0) v.x = x; else v.y = x; }
__device__ __forceinline__ void put(float4 &v, int j, float x)
{
    if (j == 0) v.x = x; else if (j == 1) v.y = x; else if (j == 2) v.z = x; else v.w = x;
}

template <class G>
__global__ void __launch_bounds__(WAVE) k_replay_batch(ReplayBatch a, int64_t per_group)
{
    using Au = Augment<G>;
    using SrcUnit = typename Au::SrcUnit;
    using OutUnit = typename Au::OutUnit;
    constexpr int S = Au::S, A = G::ACTIONS, ROW = 3 * G::CELLS;
    constexpr int SB = sizeof(SrcUnit), W = sizeof(OutUnit) / sizeof(float);
    constexpr int SRC_UNITS = ROW / SB, OUT_UNITS = ROW / W;
    constexpr int AL = A < WAVE ? A : WAVE;           // actions that ride one per lane
    constexpr bool TAIL = A > WAVE;                   // Othello's 65th action (pass): wave-uniform, never permuted
    static_assert(SRC_UNITS * SB == ROW && OUT_UNITS * W == ROW, "a state row is a whole number of loads and of stores");
    static_assert(SRC_UNITS <= WAVE && OUT_UNITS <= WAVE && A <= WAVE + 1 && 3 * S <= WAVE, "one wavefront per sample");

    const int lane = threadIdx.x;
    // Neighbouring samples write neighbouring output rows, and the narrow tensors (one to twelve bytes per row) share
    // cache lines across samples: blocks with the same blockIdx % 8 take one contiguous run of samples, so the pieces
    // of a line tend to meet in one L2.  Placement only changes speed.
    const int64_t b = static_cast<int64_t>(blockIdx.x % 8) * per_group + blockIdx.x / 8;
    if (b >= a.B) return;
    const int64_t at = a.first + b;
    const int64_t r = a.idx[a.order != nullptr ? a.order[at] : at];
    const bool ok = r >= 0 && r < a.capacity;         // wave-uniform; a row outside the ring reads nothing
    const size_t row = ok ? static_cast<size_t>(r) : 0;

    // ---- the source row, once
    const SrcUnit *src = reinterpret_cast<const SrcUnit *>(a.state) + row * SRC_UNITS;
    const uint32_t w = (ok && lane < SRC_UNITS) ? static_cast<uint32_t>(src[lane]) : 0u;
    const uint32_t *prob = reinterpret_cast<const uint32_t *>(a.prob) + row * A;     // bit patterns
    const uint8_t *mask = a.valid_mask + row * A;
    const uint32_t p = (ok && lane < AL) ? prob[lane] : 0u;
    const uint32_t m = (ok && lane < AL) ? (mask[lane] != 0 ? 1u : 0u) : 0u;
    const uint32_t p_tail = (TAIL && ok) ? prob[A - 1] : 0u;
    const uint32_t m_tail = (TAIL && ok) ? (mask[A - 1] != 0 ? 1u : 0u) : 0u;
    const int8_t win = ok ? a.winner[row] : 0;
    const int16_t steps = ok ? a.steps_to_end[row] : 0, aux = ok ? a.aux_target[row] : 0;
    const int c3 = lane % 3;
    const uint32_t wdl = ok ? reinterpret_cast<const uint32_t *>(a.root_wdl)[row * 3 + c3] : 0u;
    const uint32_t fut = ok ? reinterpret_cast<const uint32_t *>(a.future_root_wdl)[row * 3 + c3] : 0u;

    // ---- every symmetry's row
    const int u = lane < OUT_UNITS ? lane : OUT_UNITS - 1;       // the shuffles run in every lane
    const int act = lane < AL ? lane : AL - 1;
    OutUnit *o_state = reinterpret_cast<OutUnit *>(a.o_state);
    uint32_t *o_prob = reinterpret_cast<uint32_t *>(a.o_prob);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const size_t out = static_cast<size_t>(s) * static_cast<size_t>(a.B) + static_cast<size_t>(b);
        OutUnit v;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int f = u * W + j, plane = f / G::CELLS, cell = f % G::CELLS;
            const int o = plane * G::CELLS + (plane < 2 ? Au::cell(s, cell) : cell);     // the turn plane stays
            const uint32_t unit = __shfl(w, o / SB, WAVE);
            put(v, j, static_cast<float>(static_cast<int8_t>(unit >> (8 * (o % SB)))));
        }
        if (lane < OUT_UNITS) o_state[out * OUT_UNITS + lane] = v;
        const int from = Au::action(s, act);
        const uint32_t ps = __shfl(p, from, WAVE), ms = __shfl(m, from, WAVE);
        if (lane < AL) {
            o_prob[out * A + lane] = ps;
            a.o_valid_mask[out * A + lane] = static_cast<uint8_t>(ms);
        }
        if (TAIL && lane == 0) {
            o_prob[out * A + A - 1] = p_tail;
            a.o_valid_mask[out * A + A - 1] = static_cast<uint8_t>(m_tail);
        }
    }
    // ---- the columns that no symmetry touches: lane -> (symmetry, component)
    if (lane < 3 * S) {
        const size_t out = static_cast<size_t>(lane / 3) * static_cast<size_t>(a.B) + static_cast<size_t>(b);
        reinterpret_cast<uint32_t *>(a.o_root_wdl)[out * 3 + c3] = wdl;
        reinterpret_cast<uint32_t *>(a.o_future_root_wdl)[out * 3 + c3] = fut;
        if (c3 == 0) {
            a.o_winner[out] = win;
            a.o_steps_to_end[out] = steps;
            a.o_aux_target[out] = aux;
        }
    }
}

constexpr int INDEX_THREADS = 256;

// Element e of call `call`: one 64-bit draw d from the stream (seed, call, e, REPLAY_STREAM), index = the high
// half of d * n_valid (a multiply-high, no division).  Of the 2^64 values of d each index receives floor or ceil
// of 2^64 / n_valid, so its probability is off 1 / n_valid by less than 2^-64: a relative bias below n_valid / 2^64
// (under 3e-14 for a ring of 500 000 rows).
__global__ void __launch_bounds__(INDEX_THREADS) k_replay_indices(uint64_t seed, uint64_t call, uint64_t n_valid, int64_t *idx, int64_t n)
{
    const int64_t e = static_cast<int64_t>(blockIdx.x) * INDEX_THREADS + threadIdx.x;
    if (e >= n) return;
    DevRng rng(seed, call, static_cast<uint64_t>(e), REPLAY_STREAM);
    const uint64_t hi = rng.next(), lo = rng.next();
    idx[e] = static_cast<int64_t>(__umul64hi((hi << 32) | lo, n_valid));
}

}  // namespace

int replay_num_augment(int game)
{
    return game == Connect4Dev::GAME_ID ? Augment<Connect4Dev>::S : Augment<OthelloDev>::S;
}

void launch_replay_batch(int game, ReplayBatch a, hipStream_t s)
{
    if (a.B <= 0) return;
    const int64_t per_group = (a.B + 7) / 8;
    const dim3 grid(static_cast<unsigned>(8 * per_group));
    if (game == Connect4Dev::GAME_ID) hipLaunchKernelGGL(k_replay_batch<Connect4Dev>, grid, dim3(WAVE), 0, s, a, per_group);
    else hipLaunchKernelGGL(k_replay_batch<OthelloDev>, grid, dim3(WAVE), 0, s, a, per_group);
}

void launch_replay_indices(uint64_t seed, uint64_t call, int64_t n_valid, int64_t *idx, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_replay_indices, dim3(static_cast<unsigned>((n + INDEX_THREADS - 1) / INDEX_THREADS)), dim3(INDEX_THREADS),
                       0, s, seed, call, static_cast<uint64_t>(n_valid), idx, n);
}

}  // namespace az
