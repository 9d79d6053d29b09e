// rollout_search.hip - k_rollout_search: a whole pure-MCTS search (BatchedMCTS::search with RolloutEvaluator,
// BatchedMCTS.h:339-407) per tree in ONE launch.  az_mcts_search_rollout_dev spends four launches on a simulation -
// k_select, k_rollout, k_backprop, k_bump_call - because a network evaluator has to run between selection and backup.
// A random playout is a function of the leaf, trees are independent, and one lane group can carry its tree through
// n_sims simulations without leaving the kernel.  Work decomposition and arithmetic: see kernels.hip.
//
// The descent restates k_select<G, false> at K = 1 and the expansion + backup k_backprop<G, false, false> at K = 1,
// operation for operation (a known duplication, DESIGN.md 6e: those two bodies are interleaved with the K loop and
// the virtual-loss branches and sit under every bit-exact fixture; tests/test_rollout_search_gpu.py holds the two
// statements equal).  What differs is where a simulation's state lives:
//   * the leaf (slot, position, flags, result) stays in registers between the three phases;
//   * the path lives one depth per lane (lane j <-> depth j, as the backup pairs them); depth j >= LANES is written
//     to LeafBuf::path by lane j mod LANES, the lane that reads it back in the backup;
//   * the launch boundary was the fence.  From one simulation to the next lanes read records that OTHER lanes of the
//     same wavefront stored (the owner lane's meta / child_off, the new children, the path's n_visits / w_*).  One
//     wavefront owns a tree throughout and a workgroup is that wavefront: a workgroup-scope release/acquire
//     (__threadfence_block) between a backup's stores and the next descent's loads.  Inside a simulation every record
//     that is read again is read by the lane that wrote it (the expanded leaf by its owner lane, spilled path entries
//     as above), or comes from registers.  The arena pointers are neither const nor __restrict__: no tree read may go
//     through the scalar cache, which this kernel's vector stores do not update.
//   * the generator's call number of simulation `it` is call0 + it, call0 = *p.call_ptr + call_off read once; the
//     counter is not written here (workgroups are not all resident at once: a late starter would read a bumped
//     value) - a one-thread launch behind the last chunk adds the whole search's simulations.
#include "tree_dev.h"

namespace az {
namespace {

template <class G>
__global__ void __launch_bounds__(WAVE) k_rollout_search(TreeArena ar, RootState rs, LeafBuf lf, SearchParams p, int n_sims,
                                                         uint64_t call_off, unsigned long long *counters, int *err)
{
    constexpr int L = G::LANES;
    constexpr int TPW = WAVE / L;
    const int lane = threadIdx.x;
    const int sub = lane % L;
    const int tree = blockIdx.x * TPW + lane / L;
    const bool live = tree < ar.B;
    const int t = live ? tree : 0;
    const float tree_ne = p.noise_eps_tree != nullptr ? p.noise_eps_tree[t] : p.noise_eps;   // root-noise epsilon of this tree
    const uint64_t call0 = *p.call_ptr + call_off;

    HotRec *hot = ar.hot + tree_base(ar, t);
    ColdRec *cold = ar.cold + tree_base(ar, t);
    const int root = ar.root[t];
    GameState rstate;
    rstate.bb0 = rs.bb0[t]; rstate.bb1 = rs.bb1[t]; rstate.turn = rs.turn[t]; rstate.aux = rs.aux[t];
    int32_t *spill = lf.path + static_cast<size_t>(t) * G::MAX_PATH;      // path entries of depths >= L
    int used = ar.used[t];
    const int used0 = used;

    unsigned n_levels = 0, n_terminal = 0, n_exp = 0, n_backup = 0;

    for (int it = 0; it < n_sims; ++it) {
        // what the previous simulation's expansion and backup stored is read by other lanes from here on
        __threadfence_block();

        // ---- descent: MCTS.h:242-322 with compute_fpu (140-156) and select_edge (163-234) across the group's lanes
        bool done = !live;
        int cur = root, cur_lane = 0, depth = 0;
        HotRec R = hot[root];
        GameState st = rstate;
        int my_slot = root;                               // this lane's path entry: depth `sub`
        bool term = false;
        int code = 0;
        uint32_t lm = 0;                                  // the leaf's flags as the expansion must find them

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
                    const float u = c_puct * eff_prior * sqrtf(parent_n) / (1.0f + static_cast<float>(child_total));
                    const float m_util = real ? G::aux_utility(child_m, parent_m, child_q, p) : 0.0f;
                    const float score = q + u + m_util;

                    // strict '>' over ascending edges == max score, lowest index on ties; NaN and -inf can never
                    // win (MCTS.h:172,226-231)
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
                        if (nm != c.meta) { c.meta = nm; hot[child_slot].meta = nm; }
                    }
                    R = group_bcast<L>(c, best);
                    cur = child_slot;
                    cur_lane = best;
                    ++depth;
                    if (depth < L) { if (sub == depth) my_slot = cur; }
                    else if (sub == depth % L) spill[depth] = cur;       // depth <= 42 plies (C4) / < OT_MAX_PATH: in range
                } else {
                    // leaf reached: MCTS.h:291-321
                    lm = R.meta;
                    term = (lm & META_TERMINAL) != 0;
                    code = static_cast<int>((lm & META_RESULT_MASK) >> META_RESULT_SHIFT);
                    if (!term) {
                        const int res = G::result(st);
                        if (res >= 0) {
                            term = true; code = res;
                            lm = (lm & ~META_RESULT_MASK) | META_TERMINAL |
                                 (static_cast<uint32_t>(res) << META_RESULT_SHIFT);
                            if (sub == cur_lane) hot[cur].meta = lm;
                        }
                    }
                    if (term) ++n_terminal;
                    done = true;
                }
            }
            if (__all(done)) break;
        }

        if (live) {
            // ---- playout (k_rollout): uniform policy, the value is the result of a random playout, auxiliary value 0.
            // Every lane of the group plays the same moves from the same stream: the result is group-uniform.
            if (!term) code = random_playout<G>(st, p.seed, call0 + static_cast<uint64_t>(it), static_cast<uint64_t>(t));
            const float wd = code == 0 ? 1.0f : 0.0f, w1 = code == 1 ? 1.0f : 0.0f, w2 = code == 2 ? 1.0f : 0.0f;
            const float ml = term ? G::terminal_aux(st, p) : 0.0f;       // MCTS.h:412,608
            const int len = depth + 1;
            const int leaf = cur;
            const int owner = (len - 1) % L;

            // ---- expansion (MCTS.h:329-375) with the policy all ones under symmetry id 0
            if (!term) {
                const int nv = G::num_valid(st);
                const int my_action = sub < nv ? G::nth_valid(st, sub) : -1;
                const float my_pol = my_action >= 0 ? 1.0f : 0.0f;
                // the ordered sum of nv ones (0 + 1 + 1 + ...) is nv exactly: no exchange needed
                const float psum = static_cast<float>(nv);
                const float prior = my_pol / (psum + 1e-8f);            // MCTS.h:370
                if (static_cast<int64_t>(used) + nv > ar.S) {
                    if (sub == 0) atomicOr(err, ERR_ARENA_OVERFLOW);    // the expansion is dropped: no store out of range
                } else {
                    const bool root_leaf = (len == 1);                  // leaf.parent == -1, MCTS.h:349
                    float noise = 0.0f;
                    if (root_leaf && p.alpha > 0.0f) {
                        if (sub < nv) {
                            DevRng g(p.seed, call0 + static_cast<uint64_t>(it), static_cast<uint64_t>(t), static_cast<uint64_t>(sub) + 16);
                            noise = g.gamma(p.alpha);
                        }
                        float sum = 0.0f;
                        if (L == WAVE) sum = wave_ordered_sum(noise, nv); else for (int i = 0; i < nv; ++i) sum += __shfl(noise, i, L);
                        noise = noise * (1.0f / (sum + 1e-8f));
                    }
                    if (sub < nv) {
                        HotRec h = empty_rec();
                        h.prior = prior; h.meta = static_cast<uint32_t>(my_action);
                        hot[used + sub] = h;
                        if (root_leaf) {                                // cold record: see k_backprop_spread
                            ColdRec cr;
                            cr.w_draw = 0.f; cr.noise = noise; cr.parent = leaf; cr.reserved = 0;
                            cold[used + sub] = cr;
                        }
                    }
                    if (sub == owner) {
                        lm = (lm & ~META_NEDGE_MASK) | META_EXPANDED | (static_cast<uint32_t>(nv) << META_NEDGE_SHIFT);
                        hot[leaf].child_off = used;
                        hot[leaf].meta = lm;
                    }
                    used += nv;
                    ++n_exp;
                }
            }

            // ---- propagate (MCTS.h:381-402), lane j <-> depth j (root = 0): the node `dist` levels above the leaf
            // receives the auxiliary value after `dist` per-ply steps (+1 or sign flip) and the value decayed dist times
            for (int j = sub; j < len; j += L) {
                const int dist = len - 1 - j;
                float a = wd, b = w1, c = w2, mm = ml;
                const float g = p.value_decay;
                const float cst = (1.0f - g) * (1.0f / 3.0f);
                for (int i = 0; i < dist; ++i) {
                    if (G::AUX_PLUS_ONE) mm += 1.0f;
                    if (G::AUX_NEGATE) mm = -mm;
                    if (g < 1.0f) { a = fmaf(a, g, cst); b = fmaf(b, g, cst); c = fmaf(c, g, cst); }
                }
                const int slot = j < L ? my_slot : spill[j];
                HotRec h = hot[slot];
                const float dr = h.n_visits != 0 ? cold[slot].w_draw : 0.0f;   // first backup through a node: zero
                h.n_visits += 1; h.w_p1 += b; h.w_p2 += c; h.m_sum += mm;
                hot[slot].n_visits = h.n_visits;
                hot[slot].w_p1 = h.w_p1; hot[slot].w_p2 = h.w_p2; hot[slot].m_sum = h.m_sum;
                cold[slot].w_draw = dr + a;
                ++n_backup;
            }
        }
    }
    if (live && sub == 0 && used != used0) ar.used[t] = used;

    // once per wavefront (every lane must arrive here: no path of this kernel returns earlier)
    wave_add_counter(counters, CNT_LEVELS, sub == 0 ? n_levels : 0u);
    wave_add_counter(counters, CNT_TERMINAL, sub == 0 ? n_terminal : 0u);
    wave_add_counter(counters, CNT_EXPANSIONS, sub == 0 ? n_exp : 0u);
    wave_add_counter(counters, CNT_BACKUP, n_backup);
    wave_add_counter(counters, CNT_SIMS, (live && sub == 0) ? static_cast<unsigned>(n_sims) : 0u);
}

}  // namespace

void launch_rollout_search(int game, TreeArena ar, RootState rs, LeafBuf lf, SearchParams p, int n_sims, uint64_t call_off,
                           unsigned long long *counters, int *err, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_rollout_search<G>, dim3(grid_for(ar.B, WAVE / G::LANES)), dim3(WAVE), 0, s, ar, rs,
                                         lf, p, n_sims, call_off, counters, err));
}

}  // namespace az
