// select_kernels.hip - the selection kernels of the batched PUCT search (work decomposition, memory-ordering rule
// and arithmetic: see kernels.hip): k_select (every game), k_select8 and k_select8x4 (Connect4's groups of 8 lanes).
#include "tree_dev.h"

namespace az {
namespace {

// ------------------------------------------------------------------ selection

// MCTS.h:242-322 (VL=false) / 443-545 (VL=true) for K consecutive descents of every tree,
// with compute_fpu (140-156) and select_edge (163-234) evaluated across the group's lanes.
template <class G, bool VL>
__global__ void __launch_bounds__(WAVE) k_select(TreeArena ar, RootState rs, LeafBuf lf, SearchParams p, int K,
                                                 int tpw, unsigned long long *counters, uint64_t *bump, long long *zero)
{
    constexpr int L = G::LANES;
    const int lane = threadIdx.x;
    // Device generator: one new call number per iteration.  Selection draws nothing, and every
    // kernel that does (gather: symmetry ids; backup: root noise - distinct streams of one call
    // number) runs after it on the stream, so the bump rides here instead of in launches of its own.
    if (bump != nullptr && blockIdx.x == 0 && lane == 0) *bump += 1;
    if (zero != nullptr && blockIdx.x == 0 && lane == 0) *zero = 0;   // the live-leaf count of this iteration
    const int sub = lane % L;
    const int grp = lane / L;
    const int tree = blockIdx.x * tpw + grp;
    const bool live = grp < tpw && tree < ar.B;
    const int t = live ? tree : 0;
    const float tree_ne = p.noise_eps_tree != nullptr ? p.noise_eps_tree[t] : p.noise_eps;   // root-noise epsilon of this tree

    HotRec *hot = ar.hot + tree_base(ar, t);
    const ColdRec *cold = ar.cold + tree_base(ar, t);
    const int root = ar.root[t];
    HotRec rootrec = hot[root];
    int root_infl = rootrec.n_inflight;
    GameState rstate;
    rstate.bb0 = rs.bb0[t]; rstate.bb1 = rs.bb1[t]; rstate.turn = rs.turn[t]; rstate.aux = rs.aux[t];

    // state of the descent in progress (uniform across the group)
    int k = 0;
    bool done = !live;
    int cur = root, cur_lane = 0, depth = 0;
    HotRec R = rootrec;
    GameState st = rstate;
    size_t flat = static_cast<size_t>(t) * K;
    int32_t *path = lf.path + flat * G::MAX_PATH;
    if (!done && sub == 0) path[0] = root;

    unsigned n_levels = 0, n_terminal = 0;

    for (;;) {
        if (!done) {
            const uint32_t meta = R.meta;
            const int E = static_cast<int>((meta & META_NEDGE_MASK) >> META_NEDGE_SHIFT);
            bool stop = !(meta & META_EXPANDED) || (meta & META_TERMINAL) || E == 0;   // MCTS.h:250-258
            int best = -1;
            HotRec c = empty_rec();
            if (!stop) {
                const bool has = sub < E;
                const bool is_root = cur == root;
                const float ne = tree_ne;
                float noise = 0.0f;
                if (has) {
                    c = hot[R.child_off + sub];
                    if (is_root && ne > 0.0f) noise = cold[R.child_off + sub].noise;
                }
                const bool exists = has && (c.meta & META_EXISTS);
                const bool real = exists && c.n_visits > 0;

                // compute_fpu: prior mass of children with real visits, summed in edge order
                const float pq = mean_q(R.n_visits, R.w_p1, R.w_p2, (meta & META_TURN_P1) != 0);
                const float seen_term = real ? c.prior : 0.0f;
                float seen = 0.0f;
                if (L <= 8) {
#pragma unroll
                    for (int i = 0; i < L - 1; ++i) seen += __shfl(seen_term, i, L);   // lanes >= E hold 0
                } else if (L == WAVE) {
                    seen = wave_ordered_sum(seen_term, E);
                } else {
                    for (int i = 0; i < E; ++i) seen += __shfl(seen_term, i, L);
                }
                const float scale = (1.0f + pq) / 2.0f;
                const float eff = p.fpu_reduction * scale;
                float fpu = fmaf(-eff, sqrtf(seen), pq);
                fpu = (-1.0f < fpu) ? fpu : -1.0f;

                // select_edge
                const int pn_i = R.n_visits + R.n_inflight;
                const float parent_n = static_cast<float>(pn_i);
                const float parent_m = mean_m(R.n_visits, R.m_sum);
                const float c_puct = (pn_i >= 0 && pn_i < p.tab_n)
                    ? p.cpuct_tab[pn_i]
                    : p.c_init + logf((parent_n + p.c_base + 1.0f) / p.c_base);
                float eff_prior = c.prior;
                if (is_root && ne > 0.0f) eff_prior = fmaf(c.prior, 1.0f - ne, ne * noise);

                float q, child_q = 0.0f, child_m = 0.0f;
                int child_total = 0;
                if (real) {
                    child_total = c.n_visits + c.n_inflight;
                    child_q = mean_q(c.n_visits, c.w_p1, c.w_p2, (c.meta & META_TURN_P1) != 0);
                    child_m = mean_m(c.n_visits, c.m_sum);
                    q = -child_q;
                } else if (exists && c.n_inflight > 0) {
                    q = fpu;
                    child_total = c.n_inflight;
                } else {
                    q = fpu;
                }
                const float u = c_puct * eff_prior * sqrtf(parent_n) /
                                (1.0f + static_cast<float>(child_total));
                const float m_util = real ? G::aux_utility(child_m, parent_m, child_q, p) : 0.0f;
                const float score = q + u + m_util;

                // strict '>' over ascending edges == max score, lowest index on ties; NaN and
                // -inf can never win (MCTS.h:172,226-231)
                if (L == WAVE) {
                    best = wave_argmax(score, has);
                } else {
                    float s = (has && score == score) ? score : -INFINITY;
                    int si = sub;
#pragma unroll
                    for (int o = L / 2; o > 0; o >>= 1) {
                        const float os = __shfl_xor(s, o, L);
                        const int oi = __shfl_xor(si, o, L);
                        if (os > s || (os == s && oi < si)) { s = os; si = oi; }
                    }
                    best = (s > -INFINITY) ? si : -1;
                }
                if (best < 0) stop = true;
            }

            if (!stop) {
                ++n_levels;
                if (VL && depth == 0) root_infl += p.vl_count;      // MCTS.h:470-475
                const int action = L == WAVE
                    ? __builtin_amdgcn_readlane(static_cast<int>(c.meta & META_ACTION_MASK), __builtin_amdgcn_readfirstlane(best))
                    : __shfl(static_cast<int>(c.meta & META_ACTION_MASK), best, L);
                G::step(st, action);
                const int res = G::result(st);
                const int child_slot = R.child_off + best;
                if (sub == best) {
                    uint32_t nm = c.meta;
                    if (!(nm & META_EXISTS))                          // lazy child, MCTS.h:268-275
                        nm = (nm & ~META_TURN_P1) | META_EXISTS | (st.turn == 1 ? META_TURN_P1 : 0u);
                    if (res >= 0)                                     // MCTS.h:279-288
                        nm = (nm & ~META_RESULT_MASK) | META_TERMINAL |
                             (static_cast<uint32_t>(res) << META_RESULT_SHIFT);
                    if (VL) {                                         // MCTS.h:492
                        c.n_inflight += p.vl_count;
                        hot[child_slot].n_inflight = c.n_inflight;
                    }
                    if (nm != c.meta) { c.meta = nm; hot[child_slot].meta = nm; }
                }
                R = group_bcast<L>(c, best);
                cur = child_slot;
                cur_lane = best;
                ++depth;
                if (sub == 0) path[depth] = cur;
            } else {
                // leaf reached: MCTS.h:291-321 / 512-544
                uint32_t lm = R.meta;
                bool term = (lm & META_TERMINAL) != 0;
                int code = static_cast<int>((lm & META_RESULT_MASK) >> META_RESULT_SHIFT);
                if (!term) {
                    const int res = G::result(st);
                    if (res >= 0) {
                        term = true; code = res;
                        lm = (lm & ~META_RESULT_MASK) | META_TERMINAL |
                             (static_cast<uint32_t>(res) << META_RESULT_SHIFT);
                        if (sub == cur_lane) hot[cur].meta = lm;
                        if (depth == 0) rootrec.meta = lm;
                    }
                }
                if (term) ++n_terminal;
                uint8_t fl = static_cast<uint8_t>((term ? LEAF_TERMINAL : 0) | (code << LEAF_RESULT_SHIFT));
                if (VL && depth > 0) fl |= LEAF_VL_APPLIED;
                if (depth == 0 && !(lm & META_EXPANDED)) fl |= LEAF_ROOT_UNEXPANDED;
                if (lm & META_EXPANDED) fl |= LEAF_EXPANDED;
                const int nv = term ? 0 : G::num_valid(st);
                if (sub == 0) lf.slot[flat] = cur;
                if (sub == 1) lf.bb0[flat] = st.bb0;
                if (sub == 2) lf.bb1[flat] = st.bb1;
                if (sub == 3) lf.turn[flat] = st.turn;
                if (sub == 4) lf.flags[flat] = fl;
                if (sub == 5) lf.path_len[flat] = depth + 1;
                if (sub == 6) lf.aux[flat] = st.aux;
                if (sub == 7) lf.nvalid[flat] = static_cast<uint8_t>(nv);

                ++k;
                if (k == K) {
                    done = true;
                } else {
                    ++flat;
                    path += G::MAX_PATH;
                    cur = root; cur_lane = 0; depth = 0;
                    R = rootrec; R.n_inflight = root_infl;
                    st = rstate;
                    if (sub == 0) path[0] = root;
                }
            }
        }
        if (__all(done)) break;
    }

    if (live && VL && sub == 0 && root_infl != rootrec.n_inflight) hot[root].n_inflight = root_infl;

    wave_add_counter(counters, CNT_LEVELS, sub == 0 ? n_levels : 0u);
    wave_add_counter(counters, CNT_TERMINAL, sub == 0 ? n_terminal : 0u);
    wave_add_counter(counters, CNT_SIMS, (live && sub == 0) ? static_cast<unsigned>(K) : 0u);
}

// ------------------------------------------------------------------ selection, Connect4-shaped groups of 8 lanes
//
// k_select run by ONE wavefront per SIMD issues every instruction - vector or scalar - at 4 cycles, so
// a level costs (instructions x 4) cycles plus its waits, and a launch ends when the wavefront with the
// deepest trees is done.  k_select's level body is ~400 instructions and its leaf path another ~430;
// the eight trees of a wavefront are out of step, so nearly every trip through its loop pays BOTH.
// This kernel computes the same search (bit-identical: both are held to the oracle by tests/test_tree_variants_gpu.py,
// AZ_SELECT_VARIANT=0 and =1) with the instruction stream cut down:
//   * a trip = one level, then - only for groups that just arrived at a leaf - a short emit; no trips
//     spent on leaves alone (levels instead of levels + K trips per tree);
//   * cross-lane traffic inside a group is DPP on the vector ALU (quad_perm / row_half_mirror compose
//     every 8-lane exchange): the ordered 7-term prior sum and the (score, lowest index) arg-max no
//     longer take five dependent trips through the LDS crossbar; the arg-max runs on an
//     order-preserving integer key and ends in one ballot;
//   * what the winner's lane holds is fetched in ONE batch of seven independent ds_bpermute; the new
//     node's flags are then computed by every lane alike instead of being computed by one and re-sent;
//   * predicated single-lane stores (a branch each) are gathered into one block per level and one per
//     leaf; the first 16 path entries ride in two registers per lane (lane j keeps depths j, j+8) and
//     leave with two unconditional stores per leaf (entries past the path's end are ignored downstream);
// (Touching the grandchildren's blocks while a level's arithmetic runs was tried and was slower: the loads
// mostly hit L2 already and the touches only add instructions.)
constexpr int DPP_QP0 = 0x00, DPP_QP1 = 0x55, DPP_QP2 = 0xAA, DPP_QP3 = 0xFF;     // quad_perm broadcasts of lane 0..3
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_QREV = 0x1B;                  // quad_perm [1,0,3,2] [2,3,0,1] [3,2,1,0]
constexpr int DPP_HALF_MIRROR = 0x141;                                            // lane i <- lane 7 - i in each 8

template <int CTRL, int BANK_MASK = 0xf>
__device__ __forceinline__ float dpp_f(float old, float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL, 0xf, BANK_MASK, false));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t x)
{
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(x), static_cast<int>(x), CTRL, 0xf, 0xf, false));
}

// ((((((0 + t0) + t1) + t2) + t3) + t4) + t5) + t6 of the group's lanes 0..6, in every lane of the group:
// the order of `for (i < 7) sum += shfl(t, i)`, i.e. of the reference's loop over edges.  Lanes 0-3 add
// their quad's four terms, the running sum crosses to lanes 4-7 mirrored, they add theirs, and the total
// crosses back into the banks of lanes 0-3.
__device__ __forceinline__ float group8_ordered_sum7(float t)
{
    float a = 0.0f + dpp_f<DPP_QP0>(t, t);
    a = a + dpp_f<DPP_QP1>(t, t);
    a = a + dpp_f<DPP_QP2>(t, t);
    a = a + dpp_f<DPP_QP3>(t, t);
    const float x = dpp_f<DPP_HALF_MIRROR>(a, a);
    float s = x + dpp_f<DPP_QP0>(t, t);
    s = s + dpp_f<DPP_QP1>(t, t);
    s = s + dpp_f<DPP_QP2>(t, t);
    return dpp_f<DPP_HALF_MIRROR, 0x5>(s, s);          // banks 0 and 2 (lanes 0-3 of each group) take lanes 7-4's total
}

// Lane of the group's largest score, the lowest one on ties; -1 if no lane is `valid` or every valid
// score is -inf (MCTS.h:172,226-231: strict '>' over ascending edges, from -inf).
__device__ __forceinline__ int group8_argmax(float score, bool valid, int lane)
{
    const float s = valid ? score + 0.0f : -INFINITY;  // -0 -> +0: the two compare equal in the reference
    const uint32_t b = __float_as_uint(s);
    const uint32_t key = b ^ (static_cast<uint32_t>(static_cast<int32_t>(b) >> 31) | 0x80000000u);   // order-preserving
    uint32_t m = max(key, dpp_u<DPP_XOR1>(key));
    m = max(m, dpp_u<DPP_XOR2>(m));
    m = max(m, dpp_u<DPP_QREV>(dpp_u<DPP_HALF_MIRROR>(m)));                                         // lane ^ 4
    const unsigned long long bal = __ballot(key == m && m != 0x007FFFFFu);                          // 0x007FFFFF = key(-inf)
    const uint32_t g = static_cast<uint32_t>(bal >> (lane & 56)) & 0xffu;
    return g ? __ffs(g) - 1 : -1;
}

template <bool VL>
__global__ void __launch_bounds__(WAVE) k_select8(TreeArena ar, RootState rs, LeafBuf lf, SearchParams p, int K,
                                                  int tpw, unsigned long long *counters, uint64_t *bump, long long *zero)
{
    using G = Connect4Dev;
    constexpr int L = 8;
    const int lane = threadIdx.x;
    if (bump != nullptr && blockIdx.x == 0 && lane == 0) *bump += 1;      // see k_select
    if (zero != nullptr && blockIdx.x == 0 && lane == 0) *zero = 0;
    const int sub = lane % L;
    const int grp = lane / L;
    const int tree = blockIdx.x * tpw + grp;
    const bool live = grp < tpw && tree < ar.B;
    const int t = live ? tree : 0;
    const float ne = p.noise_eps_tree != nullptr ? p.noise_eps_tree[t] : p.noise_eps;
    const bool root_mix = ne > 0.0f;

    HotRec *hot = ar.hot + tree_base(ar, t);
    const ColdRec *cold = ar.cold + tree_base(ar, t);
    const int root = ar.root[t];
    HotRec rootrec = hot[root];
    int root_infl = rootrec.n_inflight;
    GameState rstate;
    rstate.bb0 = rs.bb0[t]; rstate.bb1 = rs.bb1[t]; rstate.turn = rs.turn[t]; rstate.aux = rs.aux[t];

    int k = 0;
    bool done = !live;
    int cur = root, cur_lane = 0, depth = 0;
    HotRec R = rootrec;
    // the root's own means (MCTSNode.h:116-133): selection changes neither visits nor sums, so once per launch
    const float root_q = mean_q(rootrec.n_visits, rootrec.w_p1, rootrec.w_p2, (rootrec.meta & META_TURN_P1) != 0);
    const float root_m = mean_m(rootrec.n_visits, rootrec.m_sum);
    float Rq = root_q, Rm = root_m;
    GameState st = rstate;
    size_t flat = static_cast<size_t>(t) * K;
    int path0 = root, path1 = 0;                      // this lane's path entries: depths sub and sub + 8
    unsigned n_levels = 0, n_terminal = 0;

    auto is_leaf = [](uint32_t meta) {                // MCTS.h:250-258
        return !(meta & META_EXPANDED) || (meta & META_TERMINAL) || (meta & META_NEDGE_MASK) == 0;
    };
    // MCTS.h:291-321 / 512-544: what a finished descent leaves behind, then the next descent starts at the root
    auto emit = [&]() {
        uint32_t lm = R.meta;
        bool term = (lm & META_TERMINAL) != 0;
        int code = static_cast<int>((lm & META_RESULT_MASK) >> META_RESULT_SHIFT);
        if (depth == 0 && !term) {                    // a node entered by a move carries its result already (MCTS.h:279-288)
            const int res = G::result(st);
            if (res >= 0) {
                term = true; code = res;
                lm = (lm & ~META_RESULT_MASK) | META_TERMINAL | (static_cast<uint32_t>(res) << META_RESULT_SHIFT);
                if (sub == cur_lane) hot[cur].meta = lm;
                rootrec.meta = lm;
            }
        }
        if (term) ++n_terminal;
        uint8_t fl = static_cast<uint8_t>((term ? LEAF_TERMINAL : 0) | (code << LEAF_RESULT_SHIFT));
        if (VL && depth > 0) fl |= LEAF_VL_APPLIED;
        if (depth == 0 && !(lm & META_EXPANDED)) fl |= LEAF_ROOT_UNEXPANDED;
        if (lm & META_EXPANDED) fl |= LEAF_EXPANDED;
        constexpr uint64_t TOP = 0x0000810204081020ull;               // the top cell of every column
        const int nv = term ? 0 : 7 - static_cast<int>(__builtin_popcountll((st.bb0 | st.bb1) & TOP));
        int32_t *path = lf.path + flat * G::MAX_PATH;
        if (sub <= depth) path[sub] = path0;                           // entries past depth are ignored downstream: not written
        if (sub + 8 <= depth) path[sub + 8] = path1;                   // (they were 2 MB of stores per launch that nobody reads)
        if (sub == 0) {
            lf.slot[flat] = cur; lf.bb0[flat] = st.bb0; lf.bb1[flat] = st.bb1; lf.turn[flat] = st.turn;
            lf.flags[flat] = fl; lf.path_len[flat] = depth + 1; lf.aux[flat] = st.aux;
            lf.nvalid[flat] = static_cast<uint8_t>(nv);
        }
        ++k;
        if (k == K) {
            done = true;
        } else {
            ++flat;
            cur = root; cur_lane = 0; depth = 0;
            R = rootrec; R.n_inflight = root_infl;
            Rq = root_q; Rm = root_m;
            st = rstate;
            path0 = root;                                              // depth 0 in lane 0; the others are overwritten on the way
        }
    };

    while (!done && is_leaf(R.meta)) emit();          // a root that is a leaf ends all K descents where they start

    for (;;) {
        if (!done) {
            // ---- one level from the inner node R (MCTS.h:140-234 across the lanes)
            const uint32_t meta = R.meta;
            const int E = static_cast<int>((meta & META_NEDGE_MASK) >> META_NEDGE_SHIFT);
            const bool has = sub < E;
            const bool is_root = cur == root;
            HotRec c = hot[R.child_off + (has ? sub : 0)];
            float noise = 0.0f;
            if (is_root && root_mix && has) noise = cold[R.child_off + sub].noise;
            if (!has) { c.meta = 0u; c.prior = 0.0f; c.child_off = -1; }
            const bool exists = (c.meta & META_EXISTS) != 0;
            const bool real = exists && c.n_visits > 0;

            const float pq = Rq;                      // mean_q / mean_m of R: computed when R was a candidate one level up
            const float seen = group8_ordered_sum7(real ? c.prior : 0.0f);
            const float scale = (1.0f + pq) / 2.0f;
            const float eff = p.fpu_reduction * scale;
            float fpu = fmaf(-eff, sqrtf(seen), pq);
            fpu = (-1.0f < fpu) ? fpu : -1.0f;

            const int pn_i = R.n_visits + R.n_inflight;
            const float parent_n = static_cast<float>(pn_i);
            const float parent_m = Rm;
            // both table entries by one unconditional pair of loads (index 0 outside the table, then the formulas)
            const bool in_tab = static_cast<unsigned>(pn_i) < static_cast<unsigned>(p.tab_n);
            const float *tab = p.cpuct_tab + (in_tab ? pn_i : 0);
            float c_puct = tab[0], sqrt_pn = tab[p.tab_n];
            if (!in_tab) {
                c_puct = p.c_init + logf((parent_n + p.c_base + 1.0f) / p.c_base);
                sqrt_pn = sqrtf(parent_n);
            }
            float eff_prior = c.prior;
            if (is_root && root_mix) eff_prior = fmaf(c.prior, 1.0f - ne, ne * noise);

            float q = fpu, child_q = 0.0f, child_m = 0.0f;
            int child_total = (exists && c.n_inflight > 0) ? c.n_inflight : 0;
            if (real) {
                child_total = c.n_visits + c.n_inflight;
                child_q = mean_q(c.n_visits, c.w_p1, c.w_p2, (c.meta & META_TURN_P1) != 0);
                child_m = mean_m(c.n_visits, c.m_sum);
                q = -child_q;
            }
            const float u = c_puct * eff_prior * sqrt_pn / (1.0f + static_cast<float>(child_total));
            const float m_util = real ? G::aux_utility(child_m, parent_m, child_q, p) : 0.0f;
            const float score = q + u + m_util;
            const int best = group8_argmax(score, has && score == score, lane);

            if (best >= 0) {
                ++n_levels;
                if (VL && depth == 0) root_infl += p.vl_count;                 // MCTS.h:470-475
                // the winner's record, one batch of independent exchanges
                const int src = (lane & 56) + best;
                const uint32_t bmeta = static_cast<uint32_t>(__shfl(static_cast<int>(c.meta), src));
                const int b_off = __shfl(c.child_off, src);
                const int b_n = __shfl(c.n_visits, src);
                const int b_infl = __shfl(c.n_inflight, src);
                const float b_w1 = __shfl(c.w_p1, src);
                const float b_w2 = __shfl(c.w_p2, src);
                const float b_ms = __shfl(c.m_sum, src);
                Rq = __shfl(child_q, src);             // 0 without real visits, as mean_q / mean_m of such a node are
                Rm = __shfl(child_m, src);
                G::step(st, static_cast<int>(bmeta & META_ACTION_MASK));
                const int res = G::result(st);
                uint32_t nm = bmeta;
                if (!(nm & META_EXISTS))                                       // lazy child, MCTS.h:268-275
                    nm = (nm & ~META_TURN_P1) | META_EXISTS | (st.turn == 1 ? META_TURN_P1 : 0u);
                if (res >= 0)                                                  // MCTS.h:279-288
                    nm = (nm & ~META_RESULT_MASK) | META_TERMINAL | (static_cast<uint32_t>(res) << META_RESULT_SHIFT);
                const int n_infl = VL ? b_infl + p.vl_count : b_infl;          // MCTS.h:492
                const int child_slot = R.child_off + best;
                if (sub == best) {
                    if (VL) hot[child_slot].n_inflight = n_infl;
                    if (nm != bmeta) hot[child_slot].meta = nm;
                }
                R.n_visits = b_n; R.n_inflight = n_infl; R.w_p1 = b_w1; R.w_p2 = b_w2; R.m_sum = b_ms;
                R.child_off = b_off; R.meta = nm;
                cur = child_slot;
                cur_lane = best;
                ++depth;
                if (depth < 8) { if (sub == depth) path0 = cur; }
                else if (depth < 16) { if (sub == depth - 8) path1 = cur; }
                else if (sub == 0) lf.path[flat * G::MAX_PATH + depth] = cur;
            }
            // arrived at a leaf - or no edge can be chosen (all scores NaN / -inf): the node itself is the leaf
            if (best < 0 || is_leaf(R.meta)) emit();
        }
        if (__all(done)) break;
    }
    if (live && VL && sub == 0 && root_infl != rootrec.n_inflight) hot[root].n_inflight = root_infl;

    wave_add_counter(counters, CNT_LEVELS, sub == 0 ? n_levels : 0u);
    wave_add_counter(counters, CNT_TERMINAL, sub == 0 ? n_terminal : 0u);
    wave_add_counter(counters, CNT_SIMS, (live && sub == 0) ? static_cast<unsigned>(K) : 0u);
}

// The K <= 4 virtual-loss descents of a tree SIDE BY SIDE in one wavefront: descent j lives in its own
// group of 8 lanes (a tree takes 32 lanes, a wavefront holds two trees) and starts j steps after
// descent 0.  Why they may run one level apart: descent j + 1 meets
// descent j only through what j leaves on a node when it ARRIVES there (in-flight visits, the EXISTS /
// TERMINAL bits), and j arrives one step before j + 1 reads that node among its parent's children; two
// descents of a tree are never on the same level in the same step, so they never write the same record
// in the same step.  Here the descents of a step execute as lanes of the SAME instructions, so a step
// costs one level's instructions whatever K is, and a tree needs (deepest descent + K - 1) steps instead
// of the sum of its descents' depths - which is what a launch waits for: its deepest trees.  A store of
// step s is read by another lane of the same wavefront in step s + 1: vector memory operations of one
// wavefront reach its CU's L1 in program order (wavefront scope needs no cache action in the AMDGPU
// memory model); the fences below only keep the compiler from moving them.  Results are bit-identical
// to k_select / k_select8: all three are held to the oracle on the same inputs (tests/test_tree_variants_gpu.py
// test_env_selected_route_vs_oracle; this kernel also by test_hip_parity.py).  Four wavefronts per SIMD at 8192 trees.
__global__ void __launch_bounds__(WAVE) k_select8x4(TreeArena ar, RootState rs, LeafBuf lf, SearchParams p, int K,
                                                    unsigned long long *counters, uint64_t *bump, long long *zero)
{
    using G = Connect4Dev;
    const int lane = threadIdx.x;
    if (bump != nullptr && blockIdx.x == 0 && lane == 0) *bump += 1;      // see k_select
    if (zero != nullptr && blockIdx.x == 0 && lane == 0) *zero = 0;
    const int sub = lane & 7;
    const int j = (lane >> 3) & 3;                    // which descent of its tree this group runs
    const int tree = blockIdx.x * 2 + (lane >> 5);
    const bool live = tree < ar.B && j < K;
    const int t = tree < ar.B ? tree : 0;
    const float ne = p.noise_eps_tree != nullptr ? p.noise_eps_tree[t] : p.noise_eps;
    const bool root_mix = ne > 0.0f;

    HotRec *hot = ar.hot + tree_base(ar, t);
    const ColdRec *cold = ar.cold + tree_base(ar, t);
    const int root = ar.root[t];
    const HotRec rootrec = hot[root];
    GameState st;
    st.bb0 = rs.bb0[t]; st.bb1 = rs.bb1[t]; st.turn = rs.turn[t]; st.aux = rs.aux[t];

    bool done = !live;
    bool passed_root = false;                         // this descent left the root with a chosen edge (MCTS.h:470-475)
    int cur = root, cur_lane = 0, depth = 0;
    HotRec R = rootrec;
    float Rq = mean_q(rootrec.n_visits, rootrec.w_p1, rootrec.w_p2, (rootrec.meta & META_TURN_P1) != 0);   // see k_select8
    float Rm = mean_m(rootrec.n_visits, rootrec.m_sum);
    const size_t flat = static_cast<size_t>(t) * K + (j < K ? j : 0);
    int path0 = root, path1 = 0;                      // this lane's path entries: depths sub and sub + 8
    unsigned n_levels = 0, n_terminal = 0;
    HotRec cpre = rootrec;                            // lane's record of R's children block, when have_pre
    bool have_pre = false;

    auto is_leaf = [](uint32_t meta) {                // MCTS.h:250-258
        return !(meta & META_EXPANDED) || (meta & META_TERMINAL) || (meta & META_NEDGE_MASK) == 0;
    };
    auto emit = [&]() {                               // MCTS.h:512-544
        uint32_t lm = R.meta;
        bool term = (lm & META_TERMINAL) != 0;
        int code = static_cast<int>((lm & META_RESULT_MASK) >> META_RESULT_SHIFT);
        if (depth == 0 && !term) {                    // first-time terminal test of a root (MCTS.h:299-319); every descent
            const int res = G::result(st);            // of the tree finds the same, the first one records it
            if (res >= 0) {
                term = true; code = res;
                lm = (lm & ~META_RESULT_MASK) | META_TERMINAL | (static_cast<uint32_t>(res) << META_RESULT_SHIFT);
                if (j == 0 && sub == cur_lane) hot[cur].meta = lm;
            }
        }
        if (term) ++n_terminal;
        uint8_t fl = static_cast<uint8_t>((term ? LEAF_TERMINAL : 0) | (code << LEAF_RESULT_SHIFT));
        if (depth > 0) fl |= LEAF_VL_APPLIED;
        if (depth == 0 && !(lm & META_EXPANDED)) fl |= LEAF_ROOT_UNEXPANDED;
        if (lm & META_EXPANDED) fl |= LEAF_EXPANDED;
        constexpr uint64_t TOP = 0x0000810204081020ull;               // the top cell of every column
        const int nv = term ? 0 : 7 - static_cast<int>(__builtin_popcountll((st.bb0 | st.bb1) & TOP));
        int32_t *path = lf.path + flat * G::MAX_PATH;
        if (sub <= depth) path[sub] = path0;                           // entries past depth are ignored downstream: not written
        if (sub + 8 <= depth) path[sub + 8] = path1;                   // (they were 2 MB of stores per launch that nobody reads)
        if (sub == 0) {
            lf.slot[flat] = cur; lf.bb0[flat] = st.bb0; lf.bb1[flat] = st.bb1; lf.turn[flat] = st.turn;
            lf.flags[flat] = fl; lf.path_len[flat] = depth + 1; lf.aux[flat] = st.aux;
            lf.nvalid[flat] = static_cast<uint8_t>(nv);
        }
    };
    // A group runs ONE descent, and what it found stays in its registers once it is done: the leaf is written
    // out after the loop, once per wavefront, instead of in every step in which some group arrives somewhere.

    if (!done && is_leaf(R.meta)) done = true;        // a root that is a leaf: every descent ends where it starts

    for (int step = 0;; ++step) {
        // descents of this tree that have left the root already, below this one (their in-flight visits are on it)
        const unsigned long long pb = __ballot(passed_root);
        const unsigned tree_groups = static_cast<unsigned>(pb >> (lane & 32)) & 0x01010101u;
        const bool act = !done && step >= j;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (act) {
            if (depth == 0)
                R.n_inflight = rootrec.n_inflight + p.vl_count * static_cast<int>(__builtin_popcount(tree_groups & ((1u << (8 * j)) - 1u)));
            const uint32_t meta = R.meta;
            const int E = static_cast<int>((meta & META_NEDGE_MASK) >> META_NEDGE_SHIFT);
            const bool has = sub < E;
            const bool is_root = depth == 0;
            HotRec c = cpre;                          // requested while the previous step finished (below) ...
            if (!have_pre) c = hot[R.child_off + (has ? sub : 0)];    // ... except at the root
            float noise = 0.0f;
            if (is_root && root_mix && has) noise = cold[R.child_off + sub].noise;
            if (!has) { c.meta = 0u; c.prior = 0.0f; c.child_off = -1; }
            const bool exists = (c.meta & META_EXISTS) != 0;
            const bool real = exists && c.n_visits > 0;

            const float pq = Rq;                      // mean_q / mean_m of R: computed when R was a candidate one level up
            const float seen = group8_ordered_sum7(real ? c.prior : 0.0f);
            const float scale = (1.0f + pq) / 2.0f;
            const float eff = p.fpu_reduction * scale;
            float fpu = fmaf(-eff, sqrtf(seen), pq);
            fpu = (-1.0f < fpu) ? fpu : -1.0f;

            const int pn_i = R.n_visits + R.n_inflight;
            const float parent_n = static_cast<float>(pn_i);
            const float parent_m = Rm;
            // both table entries by one unconditional pair of loads (index 0 outside the table, then the formulas)
            const bool in_tab = static_cast<unsigned>(pn_i) < static_cast<unsigned>(p.tab_n);
            const float *tab = p.cpuct_tab + (in_tab ? pn_i : 0);
            float c_puct = tab[0], sqrt_pn = tab[p.tab_n];
            if (!in_tab) {
                c_puct = p.c_init + logf((parent_n + p.c_base + 1.0f) / p.c_base);
                sqrt_pn = sqrtf(parent_n);
            }
            float eff_prior = c.prior;
            if (is_root && root_mix) eff_prior = fmaf(c.prior, 1.0f - ne, ne * noise);

            float q = fpu, child_q = 0.0f, child_m = 0.0f;
            int child_total = (exists && c.n_inflight > 0) ? c.n_inflight : 0;
            if (real) {
                child_total = c.n_visits + c.n_inflight;
                child_q = mean_q(c.n_visits, c.w_p1, c.w_p2, (c.meta & META_TURN_P1) != 0);
                child_m = mean_m(c.n_visits, c.m_sum);
                q = -child_q;
            }
            const float u = c_puct * eff_prior * sqrt_pn / (1.0f + static_cast<float>(child_total));
            const float m_util = real ? G::aux_utility(child_m, parent_m, child_q, p) : 0.0f;
            const float score = q + u + m_util;
            const int best = group8_argmax(score, has && score == score, lane);

            if (best >= 0) {
                ++n_levels;
                if (depth == 0) passed_root = true;                            // MCTS.h:470-475
                const int src = (lane & 56) + best;
                const uint32_t bmeta = static_cast<uint32_t>(__shfl(static_cast<int>(c.meta), src));
                const int b_off = __shfl(c.child_off, src);
                const int b_n = __shfl(c.n_visits, src);
                const int b_infl = __shfl(c.n_inflight, src);
                const float b_w1 = __shfl(c.w_p1, src);
                const float b_w2 = __shfl(c.w_p2, src);
                const float b_ms = __shfl(c.m_sum, src);
                Rq = __shfl(child_q, src);             // 0 without real visits, as mean_q / mean_m of such a node are
                Rm = __shfl(child_m, src);
                // What the tree's next descent must find on this node when it scores it one step from now goes
                // out first: the in-flight visits (MCTS.h:492) and, for a lazy child, EXISTS + the side to move
                // (MCTS.h:268-275; a Connect4 move always hands the turn over).  Then the node's own children are
                // requested - an expanded node is never terminal, so the descent does go on there - and the move,
                // the four-in-a-row test and the path bookkeeping below run while that load is in flight.
                const int n_infl = b_infl + p.vl_count;
                const int child_slot = R.child_off + best;
                uint32_t nm = bmeta;
                if (!(nm & META_EXISTS)) nm = (nm & ~META_TURN_P1) | META_EXISTS | (st.turn == -1 ? META_TURN_P1 : 0u);
                if (sub == best) {
                    hot[child_slot].n_inflight = n_infl;
                    if (nm != bmeta) hot[child_slot].meta = nm;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         // compiler only: the stores stay above the load
                have_pre = (bmeta & META_EXPANDED) != 0 && (bmeta & META_NEDGE_MASK) != 0;
                if (have_pre) {
                    const int e_next = static_cast<int>((bmeta & META_NEDGE_MASK) >> META_NEDGE_SHIFT);
                    cpre = hot[b_off + (sub < e_next ? sub : 0)];
                }
                G::step(st, static_cast<int>(bmeta & META_ACTION_MASK));
                const int res = G::result(st);
                if (res >= 0) {                                                // MCTS.h:279-288
                    const uint32_t tm = (nm & ~META_RESULT_MASK) | META_TERMINAL | (static_cast<uint32_t>(res) << META_RESULT_SHIFT);
                    if (sub == best && tm != nm) hot[child_slot].meta = tm;
                    nm = tm;
                }
                R.n_visits = b_n; R.n_inflight = n_infl; R.w_p1 = b_w1; R.w_p2 = b_w2; R.m_sum = b_ms;
                R.child_off = b_off; R.meta = nm;
                cur = child_slot;
                cur_lane = best;
                ++depth;
                if (depth < 8) { if (sub == depth) path0 = cur; }
                else if (depth < 16) { if (sub == depth - 8) path1 = cur; }
                else if (sub == 0) lf.path[flat * G::MAX_PATH + depth] = cur;
            }
            if (best < 0 || is_leaf(R.meta)) done = true;                      // the node itself is the leaf (MCTS.h:250-258)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (__all(done)) break;
    }
    if (live) emit();

    // in-flight visits of the root: one per descent that left it (MCTS.h:470-475)
    {
        const unsigned long long pb = __ballot(passed_root);
        const unsigned tree_groups = static_cast<unsigned>(pb >> (lane & 32)) & 0x01010101u;
        const int add = p.vl_count * static_cast<int>(__builtin_popcount(tree_groups));
        if (tree < ar.B && j == 0 && sub == 0 && add != 0) hot[root].n_inflight = rootrec.n_inflight + add;
    }

    // the three work counters in one reduction: levels of a group < 2^12, one terminal flag and one simulation each
    // (8 groups per wavefront: 8 x C4_MAX_PATH levels in 16 bits, <= 8 terminal leaves and simulations in 8 bits each;
    // readlane(63) needs every lane of the wavefront here: no path of this kernel may return before this point)
    static_assert(8 * C4_MAX_PATH < 65536, "the level counter of a wavefront is a 16-bit field");
    {
        const unsigned packed = sub == 0 ? (n_levels | (n_terminal << 16) | ((live ? 1u : 0u) << 24)) : 0u;
        const unsigned tot = wave_sum_u32(packed);
        if (lane == 0) {
            unsigned long long *c = counters + (blockIdx.x % CNT_STRIPES) * CNT_N;
            if (tot & 0xffffu) atomicAdd(&c[CNT_LEVELS], static_cast<unsigned long long>(tot & 0xffffu));
            if ((tot >> 16) & 0xffu) atomicAdd(&c[CNT_TERMINAL], static_cast<unsigned long long>((tot >> 16) & 0xffu));
            if (tot >> 24) atomicAdd(&c[CNT_SIMS], static_cast<unsigned long long>(tot >> 24));
        }
    }
}

}  // namespace

const char *launch_select(int game, TreeArena ar, RootState rs, LeafBuf lf, SearchParams p, int K, bool vl,
                          unsigned long long *counters, hipStream_t s, uint64_t *bump_call, int64_t *zero)
{
    // AZ_SELECT_VARIANT: 0 = k_select (the first kernel, every game), 1 = k_select8 (Connect4) for every launch,
    // 3 (default) = k_select8x4 for virtual-loss batches of 2..4 descents, k_select8 for the rest
    static const int variant = [] { const char *e = getenv("AZ_SELECT_VARIANT"); return e ? atoi(e) : 3; }();
    if (game == Connect4Dev::GAME_ID && variant >= 3 && vl && K >= 2 && K <= 4) {
        hipLaunchKernelGGL(k_select8x4, dim3(grid_for(ar.B, 2)), dim3(WAVE), 0, s, ar, rs, lf, p, K, counters, bump_call,
                           reinterpret_cast<long long *>(zero));
        return "k_select8x4";
    }
    if (game == Connect4Dev::GAME_ID && variant >= 1) {
        const int tpw = trees_per_wave(Connect4Dev::LANES);
        const dim3 grid(grid_for(ar.B, tpw)), block(WAVE);
        if (vl) hipLaunchKernelGGL((k_select8<true>), grid, block, 0, s, ar, rs, lf, p, K, tpw, counters, bump_call, reinterpret_cast<long long *>(zero));
        else    hipLaunchKernelGGL((k_select8<false>), grid, block, 0, s, ar, rs, lf, p, K, tpw, counters, bump_call, reinterpret_cast<long long *>(zero));
        return vl ? "k_select8<true>" : "k_select8<false>";
    }
    AZ_DISPATCH(game, {
        const int tpw = trees_per_wave(G::LANES);
        const dim3 grid(grid_for(ar.B, tpw)), block(WAVE);
        if (vl) hipLaunchKernelGGL((k_select<G, true>), grid, block, 0, s, ar, rs, lf, p, K, tpw, counters, bump_call, reinterpret_cast<long long *>(zero));
        else    hipLaunchKernelGGL((k_select<G, false>), grid, block, 0, s, ar, rs, lf, p, K, tpw, counters, bump_call, reinterpret_cast<long long *>(zero));
    });
    if (game == Connect4Dev::GAME_ID) return vl ? "k_select<Connect4Dev,true>" : "k_select<Connect4Dev,false>";
    return vl ? "k_select<OthelloDev,true>" : "k_select<OthelloDev,false>";
}

}  // namespace az
