// tree_dev.h - what the tree-kernel units (kernels.hip, select_kernels.hip, backup_kernels.hip, rollout_search.hip) share: the small
// device helpers more than one of them needs and the launchers' dispatch helpers.  Everything sits in an anonymous
// namespace: each unit gets its own copy, no device code crosses translation units.
#pragma once

#include "kernels.h"

#include <cstdlib>

#include "dev_rng.h"
#include "games.h"

namespace az {
namespace {

constexpr int WAVE = 64;

// ------------------------------------------------------------------ small device helpers

__device__ __forceinline__ float mean_q(int n, float w1, float w2, bool turn_p1)
{
    // MCTSNode.h:116-125: uniform WDL (q = 0) without visits; inv = 1/N then multiply
    if (n == 0) return 0.0f;
    const float inv = 1.0f / static_cast<float>(n);
    const float p1 = w1 * inv, p2 = w2 * inv;
    return turn_p1 ? (p1 - p2) : (p2 - p1);
}

__device__ __forceinline__ float mean_m(int n, float msum)
{
    return n == 0 ? 0.0f : msum / static_cast<float>(n);   // MCTSNode.h:131-133
}

// Work counters: CNT_STRIPES copies of the CNT_N counters, one 64-byte line each; a workgroup
// adds to the copy picked by its index, the host sums the copies.  A single copy made a thousand
// wavefronts queue on three L2 atomics per launch.
__device__ __forceinline__ void wave_add_counter(unsigned long long *counters, int which, unsigned v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, WAVE);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(&counters[(blockIdx.x % CNT_STRIPES) * CNT_N + which], static_cast<unsigned long long>(v));
}

// sum over the wavefront on the DPP network (no LDS crossbar trips), the total in every lane's copy of lane 63
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
    auto mv = [](unsigned x, auto ctrl, auto rmask) {
        return static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), decltype(ctrl)::value, decltype(rmask)::value, 0xf, false));
    };
    v += mv(v, std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xf>{});     // quad_perm [1,0,3,2]
    v += mv(v, std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xf>{});     // quad_perm [2,3,0,1]
    v += mv(v, std::integral_constant<int, 0x141>{}, std::integral_constant<int, 0xf>{});    // row_half_mirror
    v += mv(v, std::integral_constant<int, 0x140>{}, std::integral_constant<int, 0xf>{});    // row_mirror
    v += mv(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});    // row_bcast:15 into rows 1 and 3
    v += mv(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});    // row_bcast:31 into rows 2 and 3
    return static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}

// sum of `term` over lanes 0..E-1 IN LANE ORDER (the reference adds in edge order: MCTS.h:145-151,343-345); lanes
// >= E must hold +0 (adding it changes nothing), so the common case is a fixed unrolled chain of 40 readlanes
__device__ __forceinline__ float wave_ordered_sum(float term, int E)
{
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 40; ++i) s += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(term), i));
    for (int i = 40; i < E; ++i) s += __shfl(term, i, WAVE);               // positions with more than 40 legal moves (imported roots)
    return s;
}

// first record of tree t's arena: the half it lives in now (tree_layout.h: two halves per tree, a
// re-rooting copies the kept subtree into the other one)
__device__ __forceinline__ size_t tree_base(const TreeArena &ar, int t)
{
    return (static_cast<size_t>(t) * 2 + ar.half[t]) * static_cast<size_t>(ar.S);
}

__device__ __forceinline__ HotRec empty_rec()
{
    HotRec c;
    c.n_visits = 0; c.n_inflight = 0; c.w_p1 = 0.f; c.w_p2 = 0.f; c.m_sum = 0.f;
    c.prior = 0.f; c.child_off = -1; c.meta = 0u;
    return c;
}

// ---- what the plain descents (k_select, k_rollout_search) share: a record sent from one lane to its group, the
// group-wide arg-max

template <int L>
__device__ __forceinline__ HotRec group_bcast(const HotRec &c, int src)
{
    HotRec r;
    r.n_visits   = __shfl(c.n_visits, src, L);
    r.n_inflight = __shfl(c.n_inflight, src, L);
    r.w_p1       = __shfl(c.w_p1, src, L);
    r.w_p2       = __shfl(c.w_p2, src, L);
    r.m_sum      = __shfl(c.m_sum, src, L);
    r.prior      = __shfl(c.prior, src, L);
    r.child_off  = __shfl(c.child_off, src, L);
    r.meta       = static_cast<uint32_t>(__shfl(static_cast<int>(c.meta), src, L));
    return r;
}

// ---- one tree per wavefront (Othello: 64 lanes, up to 33 edges): the group-wide exchanges without the LDS crossbar.
// A __shfl with a runtime lane is a ds_bpermute (address VGPR, LDS round trip, wait); in a loop bounded by the edge
// count that is one dependent round trip per edge.  With the whole wavefront as the group the source lane is
// wave-uniform, so v_readlane_b32 (a scalar result, no LDS) does it, and reductions run on the DPP network.

// maximum of an unsigned key over the wavefront (0 = the identity of lanes switched off)
__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
    auto mv = [](unsigned x, auto ctrl, auto rmask) {
        return static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), decltype(ctrl)::value, decltype(rmask)::value, 0xf, false));
    };
    auto mx = [](unsigned a, unsigned b) { return a > b ? a : b; };
    v = mx(v, mv(v, std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xf>{}));     // quad_perm [1,0,3,2]
    v = mx(v, mv(v, std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xf>{}));     // quad_perm [2,3,0,1]
    v = mx(v, mv(v, std::integral_constant<int, 0x141>{}, std::integral_constant<int, 0xf>{}));    // row_half_mirror
    v = mx(v, mv(v, std::integral_constant<int, 0x140>{}, std::integral_constant<int, 0xf>{}));    // row_mirror
    v = mx(v, mv(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{}));    // row_bcast:15 into rows 1 and 3
    v = mx(v, mv(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{}));    // row_bcast:31 into rows 2 and 3
    return static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}
// strict '>' over ascending edges == highest score, lowest lane on ties; NaN and -inf never win (MCTS.h:172,226-231):
// an order-preserving integer key of the score (0 for lanes that cannot win), its wave-wide maximum, the lowest lane
// that holds it.  Returns -1 when no lane can win.
__device__ __forceinline__ int wave_argmax(float score, bool can_win)
{
    const uint32_t b = __float_as_uint(score);
    uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);             // monotone in the float order; -inf -> 0x007fffff
    if (!can_win || !(score > -INFINITY)) key = 0u;                         // NaN fails the comparison too
    const unsigned mx = wave_max_u32(key);
    if (mx == 0u) return -1;
    const unsigned long long hit = __ballot(key == mx);
    return static_cast<int>(__builtin_ctzll(hit));
}
template <>
__device__ __forceinline__ HotRec group_bcast<WAVE>(const HotRec &c, int src)
{
    const int u = __builtin_amdgcn_readfirstlane(src);                      // the winner's lane is the same in every lane
    HotRec r;
    r.n_visits   = __builtin_amdgcn_readlane(c.n_visits, u);
    r.n_inflight = __builtin_amdgcn_readlane(c.n_inflight, u);
    r.w_p1       = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.w_p1), u));
    r.w_p2       = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.w_p2), u));
    r.m_sum      = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.m_sum), u));
    r.prior      = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.prior), u));
    r.child_off  = __builtin_amdgcn_readlane(c.child_off, u);
    r.meta       = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(c.meta), u));
    return r;
}

// RolloutEvaluator::evaluate_single (RolloutEvaluator.h:23-48): the result - 0 draw, 1 P1 wins, 2 P2 wins - of a
// uniformly random playout from the non-terminal position `s`, moves from the device generator's playout stream
// (b = 3) of (seed, call, tree); at most 4 * CELLS plies (a position without a result by then counts as a draw)
template <class G>
__device__ __forceinline__ int random_playout(GameState s, uint64_t seed, uint64_t call, uint64_t tree)
{
    DevRng g(seed, call, tree, 3);
    int res = G::result(s);
    for (int ply = 0; res < 0 && ply < 4 * G::CELLS; ++ply) {
        const int nv = G::num_valid(s);
        if (nv <= 0) break;
        const int pick = static_cast<int>((static_cast<uint64_t>(g.next()) * static_cast<uint64_t>(nv)) >> 32);
        G::step(s, G::nth_valid(s, pick));
        res = G::result(s);
    }
    return res < 0 ? 0 : res;
}

// ------------------------------------------------------------------ launch helpers (host)

inline unsigned grid_for(int B, int trees_per_wg) { return static_cast<unsigned>((B + trees_per_wg - 1) / trees_per_wg); }

// Trees per wavefront for Connect4's two heavy kernels (AZ_TREES_PER_WAVE, default 8 = all lanes
// busy).  Measured on MI355X at 8192 trees, K=4 (hash evaluator): 8 -> 75.6 us per selection
// launch, 4 -> 96.4, 2 -> 142.4, 1 -> 236.5: the kernels are bound by instruction issue and
// dependent-instruction latency, not by memory latency, so spreading the trees over more
// wavefronts only multiplies the instruction count.
inline int trees_per_wave(int lanes)
{
    static const int v = [] {
        const char *e = getenv("AZ_TREES_PER_WAVE");
        int t = e ? atoi(e) : 8;
        return (t == 1 || t == 2 || t == 4 || t == 8) ? t : 8;
    }();
    const int max_tpw = WAVE / lanes;
    return v < max_tpw ? v : max_tpw;
}

#define AZ_DISPATCH(game, ...)                                                     \
    do {                                                                           \
        if ((game) == Connect4Dev::GAME_ID) { using G = Connect4Dev; __VA_ARGS__; } \
        else { using G = OthelloDev; __VA_ARGS__; }                                 \
    } while (0)

}  // namespace
}  // namespace az
