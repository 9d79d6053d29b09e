// sp_pick.h - the move pick shared by the ply tails of the self-play driver (selfplay_kernels.hip, k_sp_pick) and of
// the evaluation-match driver (match_kernels.hip, k_match_ply): root visit counts of one game, spread over its lane
// group, -> the move (player.py:348-371; pipeline.py:337-351 is the same rule).  Lane e of a group owns action e,
// Othello's 65th action (pass) rides with lane 0.
#pragma once

#include "dev_rng.h"
#include "games.h"

namespace az {

template <int L>
__device__ __forceinline__ unsigned long long group_ballot(bool pred, int lane)
{
    const unsigned long long bal = __ballot(pred);
    constexpr unsigned long long mask = L >= 64 ? ~0ull : ((1ull << (L & 63)) - 1ull);
    return (bal >> (lane - lane % L)) & mask;
}

template <int L, class T>
__device__ __forceinline__ T group_max(T v)
{
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) {
        const T w = __shfl_xor(v, o, L);
        v = w > v ? w : v;
    }
    return v;
}

template <int L>
__device__ __forceinline__ long long group_sum(long long v)
{
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, L);
    return v;
}

// inclusive prefix sum over the lane group, in lane order
template <int L>
__device__ __forceinline__ float group_scan(float v, int sub)
{
#pragma unroll
    for (int o = 1; o < L; o <<= 1) {
        const float w = __shfl_up(v, o, L);
        if (sub >= o) v += w;
    }
    return v;
}

// what a lane holds of its game's count row (k_sp_pick's trajectory row reads them again)
struct PickLane {
    int n0, n1;             // counts of action sub and (Othello, lane 0) action sub + L, clamped at 0
    bool has0, has1;
    long long total;        // the row's sum, the same in every lane of the group
};

// The move of game g, the same value in every lane of its group.  c0, c1: what this lane holds of the game's count
// row - action sub and (Othello, lane 0) action sub + L - read where has0 / has1 of the result say so; tape: this
// ply's recorded actions [n] or nullptr; draws come from the generator stream (seed, call, g, STREAM).
template <class G, uint64_t STREAM>
__device__ __forceinline__ int pick_move_counts(int c0, int c1, bool live, int lane, float temp, const int32_t *tape,
                                                uint64_t seed, uint64_t call, int64_t g, PickLane &pl)
{
    constexpr int L = G::LANES, A = G::ACTIONS;
    constexpr bool TWO = A > L;                       // a second action per lane (Othello: lane 0, the pass)
    const int sub = lane % L;
    const bool has0 = live && sub < A, has1 = TWO && live && sub + L < A;
    const int n0 = has0 ? max(c0, 0) : 0;
    const int n1 = has1 ? max(c1, 0) : 0;
    const long long total = group_sum<L>(static_cast<long long>(n0) + n1);
    pl.n0 = n0; pl.n1 = n1; pl.has0 = has0; pl.has1 = has1; pl.total = total;
    int action;
    if (tape != nullptr) {
        action = tape[g];
    } else if (total == 0) {
        action = 0;                                    // player.py:355-358
    } else if (!(temp > 1e-6f)) {
        // the FIRST maximal count (np.argmax): largest (count, -action)
        long long key = has0 ? ((static_cast<long long>(n0) << 8) | (255 - sub)) : -1;
        if (has1) { const long long k1 = (static_cast<long long>(n1) << 8) | (255 - (sub + L)); key = k1 > key ? k1 : key; }
        key = group_max<L>(key);
        action = 255 - static_cast<int>(key & 255);
    } else {
        // player.py:365-368: weights exp((log N - max log N) / T) over the actions with N > 0, ascending;
        // one uniform, inverse CDF
        const float ninf = -__builtin_inff();
        const float l0 = n0 > 0 ? logf(static_cast<float>(n0)) : ninf;
        const float l1 = n1 > 0 ? logf(static_cast<float>(n1)) : ninf;
        const float mx = group_max<L>(l0 > l1 ? l0 : l1);
        const float w0 = n0 > 0 ? expf((l0 - mx) / temp) : 0.0f;
        const float w1 = n1 > 0 ? expf((l1 - mx) / temp) : 0.0f;
        const float c0 = group_scan<L>(w0, sub);
        const float tot0 = __shfl(c0, L - 1, L);
        float c1 = 0.0f, tot = tot0;
        if (TWO) {
            c1 = tot0 + group_scan<L>(w1, sub);
            tot = __shfl(c1, L - 1, L);
        }
        DevRng rng(seed, call, static_cast<uint64_t>(g), STREAM);
        const float target = rng.uniform() * tot;
        const unsigned long long v0 = group_ballot<L>(n0 > 0, lane), v1 = group_ballot<L>(n1 > 0, lane);
        const unsigned long long h0 = group_ballot<L>(n0 > 0 && c0 > target, lane);
        const unsigned long long h1 = group_ballot<L>(n1 > 0 && c1 > target, lane);
        if (h0) action = __ffsll(static_cast<long long>(h0)) - 1;
        else if (h1) action = L + __ffsll(static_cast<long long>(h1)) - 1;
        else if (v1) action = L + 63 - __clzll(static_cast<long long>(v1));     // rounding left the target at the total
        else action = 63 - __clzll(static_cast<long long>(v0));
    }
    return action;
}

// pick_move_counts on a count row in memory (cnt: the game's row)
template <class G, uint64_t STREAM>
__device__ __forceinline__ int pick_move(const int32_t *cnt, bool live, int lane, float temp, const int32_t *tape,
                                         uint64_t seed, uint64_t call, int64_t g, PickLane &pl)
{
    constexpr int L = G::LANES, A = G::ACTIONS;
    const int sub = lane % L;
    const int c0 = (live && sub < A) ? cnt[sub] : 0;
    const int c1 = (A > L && live && sub + L < A) ? cnt[sub + L] : 0;
    return pick_move_counts<G, STREAM>(c0, c1, live, lane, temp, tape, seed, call, g, pl);
}

}  // namespace az
