// kernels.hip - gfx950 kernels of the batched PUCT search, instantiated per game (games.h).  Three units over
// tree_dev.h: select_kernels.hip (selection), backup_kernels.hip (virtual-loss removal, expansion + backup) and this
// one (import, leaf export, tree maintenance, root queries, rollout, game step, the device driver's ply tail).  What
// follows holds for all three.
//
// Work decomposition: ONE TREE PER LANE GROUP of G::LANES lanes (Connect4: 8 lanes, 8 trees
// per 64-wide wavefront; Othello: 64 lanes, one tree per wavefront), one wavefront per
// workgroup (no LDS, no barriers: all cross-lane traffic is group-wide shuffles).  Lane e of a
// group owns edge e of whatever node the group is looking at, so a PUCT step is
//   1 coalesced load of E adjacent 32-byte child records (tree_layout.h)
//   an E-term ordered prior sum + log2(LANES)-step (score, index) max over the group
//   <= 2 dword stores by the winning lane (in-flight count, lazily set flags).
// Trees are independent (reference: one MCTS object per env under `omp parallel for`,
// BatchedMCTS.h:107-332), so there is no inter-group or inter-workgroup communication at all.
// The K virtual-loss descents of one tree are sequential, exactly as in the reference
// (BatchedMCTS.h:249-285); groups of a wave do not wait for each other between descents.
//
// Memory-ordering rule used throughout: a record that is re-read later in the same kernel is
// always re-read by the SAME LANE that wrote it (lane = index in its sibling block for
// selection, lane = depth mod LANES for backup), so plain program order is sufficient.
//
// Arithmetic: compiled with -ffp-contract=off; IEEE fp32 divide and sqrt.  The expression
// order of MCTS.h:140-234,329-402 and MCTSNode.h:116-133 is kept, and the three fused
// multiply-adds the compiled reference contains (FPU value, root prior/noise mix, value
// decay - see oracle/mcts_impl.inc) are explicit fmaf().  No MFMA: this is index/bit work.
#include "tree_dev.h"

namespace az {
namespace {

// ------------------------------------------------------------------ import (host entry points)

template <class G>
__global__ void __launch_bounds__(256) k_import(const int8_t *boards, const int32_t *turns, RootState rs, int B)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B) return;
    GameState s;
    s.turn = turns[t];
    G::import_cells(boards + static_cast<size_t>(t) * G::CELLS, s);
    rs.bb0[t] = s.bb0; rs.bb1[t] = s.bb1; rs.turn[t] = s.turn; rs.aux[t] = s.aux;
}

// device-resident roots: the game's small integer is derived as an import would derive it
template <class G>
__global__ void __launch_bounds__(256) k_set_roots(const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns,
                                                   RootState rs, int B)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B) return;
    const uint64_t a = bb0[t], b = bb1[t];
    rs.bb0[t] = a; rs.bb1[t] = b; rs.turn[t] = turns[t];
    rs.aux[t] = G::root_aux(a, b);
}

// ------------------------------------------------------------------ leaf gather

// BatchedMCTS.h:141-169 / 254-283 (symmetry, grid export, valid mask) and MCTS_cpp.py:15-20
// (relative feature planes).  One thread per (leaf, cell); cells of a leaf are contiguous so
// every plane row is a coalesced store.
template <class G>
__global__ void __launch_bounds__(256) k_export(LeafBuf lf, SearchParams p, int n_leaves, int gen_sym,
                                                int8_t *boards, uint8_t *valid_mask, float *features)
{
    constexpr int CELLS = G::CELLS, A = G::ACTIONS;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t leaf = gid / CELLS;
    const int cell = static_cast<int>(gid - leaf * CELLS);
    if (leaf >= n_leaves) return;
    GameState s;
    s.bb0 = lf.bb0[leaf]; s.bb1 = lf.bb1[leaf]; s.turn = lf.turn[leaf]; s.aux = lf.aux[leaf];
    const bool term = (lf.flags[leaf] & LEAF_TERMINAL) != 0;
    int sym;
    if (gen_sym) {
        sym = 0;
        if (!term && p.use_symmetry) {
            DevRng g(p.seed, *p.call_ptr, static_cast<uint64_t>(leaf), 7);
            sym = G::sym_of_choice(static_cast<int>((static_cast<uint64_t>(g.next()) * G::SYM_CHOICES) >> 32));
        }
        if (cell == 0) lf.sym[leaf] = sym;
    } else {
        sym = lf.sym[leaf];
    }
    const int v = G::cell_value(s, sym, cell);
    if (boards) boards[leaf * CELLS + cell] = static_cast<int8_t>(v);
    if (features) {
        float *f = features + leaf * (3 * CELLS) + cell;
        f[0] = (v == s.turn) ? 1.0f : 0.0f;
        f[CELLS] = (v == -s.turn) ? 1.0f : 0.0f;
        f[2 * CELLS] = static_cast<float>(s.turn);
    }
    if (valid_mask) {
        for (int a = cell; a < A; a += CELLS)
            valid_mask[leaf * A + a] = (!term && G::valid_in_frame(s, sym, a)) ? 1 : 0;
    }
}

// What the native loop needs between a selection and its evaluator when the evaluator reads leaf POSITIONS
// (az_nn_model_forward_positions) instead of feature planes: the symmetry id every non-terminal leaf is shown
// under (BatchedMCTS.h:148-154), its action mask in that frame, and the compact list of the leaves to
// evaluate (everything but terminal leaves, MCTS_cpp.py:275-297) - k_export's ids and mask and
// k_live_leaves' list in one pass of one thread per leaf, with no feature tensor written or read.
template <class G>
__global__ void __launch_bounds__(1024) k_leaf_prep(LeafBuf lf, SearchParams p, int n_leaves, int gen_sym,
                                                    uint8_t *valid_mask, int32_t *idx, long long *count, int *err)
{
    constexpr int A = G::ACTIONS;
    __shared__ int s_wave[16];
    __shared__ long long s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t leaf = static_cast<int64_t>(blockIdx.x) * blockDim.x + tid;
    bool livel = false;
    if (leaf < n_leaves) {
        GameState s;
        s.bb0 = lf.bb0[leaf]; s.bb1 = lf.bb1[leaf]; s.turn = lf.turn[leaf]; s.aux = lf.aux[leaf];
        const bool term = (lf.flags[leaf] & LEAF_TERMINAL) != 0;
        livel = !term;
        int sym;
        if (gen_sym) {
            sym = 0;
            if (!term && p.use_symmetry) {                         // the draw of k_export, leaf for leaf
                DevRng g(p.seed, *p.call_ptr, static_cast<uint64_t>(leaf), 7);
                sym = G::sym_of_choice(static_cast<int>((static_cast<uint64_t>(g.next()) * G::SYM_CHOICES) >> 32));
            }
            lf.sym[leaf] = sym;
        } else {
            sym = lf.sym[leaf];
        }
        if (valid_mask != nullptr)
            for (int a = 0; a < A; ++a) valid_mask[leaf * A + a] = (!term && G::valid_in_frame(s, sym, a)) ? 1 : 0;
    }
    if (idx == nullptr) return;                                    // uniform: the table's lookup builds the list
    const unsigned long long m = __ballot(livel);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int c = s_wave[w];
        if (w < wave) before += c;
        total += c;
    }
    if (tid == 0)
        s_base = total ? static_cast<long long>(atomicAdd(reinterpret_cast<unsigned long long *>(count),
                                                          static_cast<unsigned long long>(total))) : 0;
    __syncthreads();
    if (livel) {
        const long long pos = s_base + before + __popcll(m & ((1ull << lane) - 1));
        if (pos >= 0 && pos < n_leaves) idx[pos] = static_cast<int32_t>(leaf);
        else atomicOr(err, ERR_LIST_OVERFLOW);
    }
}

// ------------------------------------------------------------------ tree maintenance

__device__ __forceinline__ void write_fresh_root(HotRec *hot, ColdRec *cold)
{
    HotRec h = empty_rec();                                            // MCTS.h:77-82
    h.meta = META_TURN_P1 | META_EXISTS;
    hot[0] = h;
    ColdRec c;
    c.w_draw = 0.f; c.noise = 0.f; c.parent = -1; c.reserved = 0;
    cold[0] = c;
}

__global__ void __launch_bounds__(256) k_init_trees(TreeArena ar)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ar.B) return;
    write_fresh_root(ar.hot + tree_base(ar, t), ar.cold + tree_base(ar, t));
    ar.root[t] = 0;
    ar.used[t] = 1;
}

__global__ void __launch_bounds__(256) k_reset_masked(TreeArena ar, const uint8_t *mask)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ar.B || !mask[t]) return;
    write_fresh_root(ar.hot + tree_base(ar, t), ar.cold + tree_base(ar, t));
    ar.root[t] = 0;
    ar.used[t] = 1;
}

// group-local ballot: bit i set <=> lane i of this lane group votes true
template <int L>
__device__ __forceinline__ unsigned long long group_ballot(bool pred, int lane)
{
    const unsigned long long bal = __ballot(pred);
    constexpr unsigned long long mask = L >= 64 ? ~0ull : ((1ull << (L & 63)) - 1ull);
    return (bal >> (lane - lane % L)) & mask;
}

// One node's child block (nE records at `src` of the old half) to `dst` of the new half, parent = q: CH records
// are loaded before the first of them is stored, so a lane waits for one memory round trip per CH records, not
// one per record (Connect4: CH = ACTIONS, a whole block; Othello: chunks of 8, which bounds the registers).
template <int CH>
__device__ __forceinline__ void copy_child_block(const HotRec *__restrict__ hot, const ColdRec *__restrict__ cold,
                                                 HotRec *__restrict__ nhot, ColdRec *__restrict__ ncold, int src, int dst,
                                                 int nE, int q)
{
    typedef uint4 __attribute__((may_alias)) rec4;                     // a record's dwordx4 halves, whatever their fields
    static_assert(sizeof(HotRec) == 2 * sizeof(rec4) && sizeof(ColdRec) == sizeof(rec4) && offsetof(ColdRec, parent) == 8,
                  "records as dwordx4, parent in .z");
    for (int j0 = 0; j0 < nE; j0 += CH) {
        const rec4 *hs = reinterpret_cast<const rec4 *>(hot + src + j0);
        const rec4 *cs = reinterpret_cast<const rec4 *>(cold + src + j0);
        rec4 *hd = reinterpret_cast<rec4 *>(nhot + dst + j0);
        rec4 *cd = reinterpret_cast<rec4 *>(ncold + dst + j0);
        const int m = nE - j0;                                         // records of this chunk: k < m
        uint4 ha[CH], hb[CH], cb[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            ha[k] = hb[k] = cb[k] = make_uint4(0u, 0u, 0u, 0u);
            if (k < m) { ha[k] = hs[2 * k]; hb[k] = hs[2 * k + 1]; cb[k] = cs[k]; }
        }
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (k < m) {
                cb[k].z = static_cast<unsigned>(q);                    // ColdRec::parent
                hd[2 * k] = ha[k]; hd[2 * k + 1] = hb[k]; cd[k] = cb[k];
            }
    }
}

// MCTS.h:90-132: re-root at the child reached by `action` if the reference would have allocated it,
// else reset.  The reference keeps the whole old tree in its pools until the next reset
// (MCTS.h:100-101: only `root_idx` moves); here the KEPT SUBTREE IS COPIED into the tree's other
// arena half, breadth first, and the tree continues there: what a tree occupies is what is
// reachable from its root (node numbering is not observable through the API; the order of records
// inside a sibling block - the edge order - is kept).  One wavefront per tree: a pass takes the
// records appended by the previous pass (64 at a time), a wave-wide prefix sum of their edge counts
// places their child blocks behind what is there, every lane copies its node's block.  Stores of a
// pass are read by other lanes of the same wavefront in the next one (wavefront-scope order, as in
// k_select8x4; the fence also drains the stores).  noise_req[t] = number of root edges that need
// fresh Dirichlet noise (host generator); with dev_noise the noise is written here, from the device
// generator or from `replay_noise`.  max_live: running maximum of the records a tree occupies now.
template <class G>
__global__ void __launch_bounds__(WAVE) k_prune(TreeArena ar, SearchParams p, const int32_t *actions,
                                                int32_t *noise_req, int dev_noise, const float *replay_noise,
                                                int *max_live, int *err, int compact_above)
{
    const int lane = threadIdx.x;
    const int t = blockIdx.x;
    const int S = static_cast<int>(ar.S);
    const int h = ar.half[t];
    // the two halves of a tree never overlap, nor do the hot and the cold arena
    HotRec *__restrict__ hot = ar.hot + (static_cast<size_t>(t) * 2 + h) * ar.S;
    ColdRec *__restrict__ cold = ar.cold + (static_cast<size_t>(t) * 2 + h) * ar.S;
    HotRec *__restrict__ nhot = ar.hot + (static_cast<size_t>(t) * 2 + (1 - h)) * ar.S;
    ColdRec *__restrict__ ncold = ar.cold + (static_cast<size_t>(t) * 2 + (1 - h)) * ar.S;
    const int root = ar.root[t];
    const HotRec R = hot[root];
    const int action = actions[t];
    const int E = (R.meta & META_EXPANDED) ? static_cast<int>((R.meta & META_NEDGE_MASK) >> META_NEDGE_SHIFT) : 0;
    HotRec c = empty_rec();
    bool match = false;
    if (lane < E) {
        c = hot[R.child_off + lane];
        match = static_cast<int>(c.meta & META_ACTION_MASK) == action && (c.meta & META_EXISTS);
    }
    const unsigned long long mb = __ballot(match);
    if (!mb) {                                                         // MCTS.h:107: reset()
        if (lane == 0) {
            write_fresh_root(hot, cold);
            ar.root[t] = 0;
            ar.used[t] = 1;
            if (!dev_noise) noise_req[t] = 0;
            atomicMax(max_live, 1);
        }
        return;
    }
    const int e = __ffsll(mb) - 1;
    const int old_root = R.child_off + e;
    // A tree that still has room for the plies to come stays where it is - the root moves to the chosen
    // record, as in the reference (MCTS.h:100-101) - and only a tree past `compact_above` records pays
    // for the copy: every few plies instead of every ply.
    if (ar.used[t] <= compact_above) {
        const uint32_t nm = static_cast<uint32_t>(__shfl(static_cast<int>(c.meta), e, WAVE));
        const int noff0 = __shfl(c.child_off, e, WAVE);
        const int nE0 = (nm & META_EXPANDED) ? static_cast<int>((nm & META_NEDGE_MASK) >> META_NEDGE_SHIFT) : 0;
        if (lane == 0) {
            ar.root[t] = old_root;
            cold[old_root].parent = -1;
            atomicMax(max_live, ar.used[t]);
        }
        const int want0 = (p.alpha > 0.0f) ? nE0 : 0;                   // apply_root_noise, MCTS.h:113-132
        if (want0 == 0 && lane < nE0) cold[noff0 + lane].noise = 0.0f;  // expansion writes the noise of the root's children only
        if (!dev_noise) {
            if (lane == 0) noise_req[t] = want0;
        } else if (want0 > 0 && replay_noise != nullptr) {
            if (lane < want0) cold[noff0 + lane].noise = replay_noise[static_cast<size_t>(t) * G::ACTIONS + lane];
        } else if (want0 > 0) {
            float g = 0.0f;
            if (lane < want0) {
                DevRng rng(p.seed, *p.call_ptr, static_cast<uint64_t>(t), static_cast<uint64_t>(lane) + 128);
                g = rng.gamma(p.alpha);
            }
            const float sum = wave_ordered_sum(g, want0);   // lanes >= want0 hold 0
            if (lane < want0) cold[noff0 + lane].noise = g * (1.0f / (sum + 1e-8f));
        }
        return;
    }
    if (lane == 0) {
        nhot[0] = hot[old_root];
        ColdRec cr = cold[old_root];
        cr.parent = -1;                                                // MCTS.h:100-101
        ncold[0] = cr;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    int lo = 0, hi = 1, used = 1;
    bool overflow = false;
    while (lo < hi && !overflow) {
        for (int q0 = lo; q0 < hi; q0 += WAVE) {
            const int q = q0 + lane;
            const bool valid = q < hi;
            HotRec rec = empty_rec();
            if (valid) rec = nhot[q];                                  // still points at its OLD child block
            const int nE = (valid && (rec.meta & META_EXPANDED)) ? static_cast<int>((rec.meta & META_NEDGE_MASK) >> META_NEDGE_SHIFT) : 0;
            int incl = nE;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const int v = __shfl_up(incl, o, WAVE);
                if (lane >= o) incl += v;
            }
            const int total = __shfl(incl, WAVE - 1, WAVE);
            if (used + total > S) { overflow = true; break; }         // cannot happen: the subtree fitted in one half before
            if (nE > 0) {
                const int dst = used + incl - nE;
                nhot[q].child_off = dst;
                copy_child_block<(G::ACTIONS < 8 ? G::ACTIONS : 8)>(hot, cold, nhot, ncold, rec.child_off, dst, nE, q);
            }
            used += total;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        lo = hi; hi = used;
    }
    if (overflow && lane == 0) atomicOr(err, ERR_ARENA_OVERFLOW);
    const HotRec NR = nhot[0];
    const int nE = (NR.meta & META_EXPANDED) ? static_cast<int>((NR.meta & META_NEDGE_MASK) >> META_NEDGE_SHIFT) : 0;
    const int noff = NR.child_off;
    if (lane == 0) {
        ar.half[t] = static_cast<uint8_t>(1 - h);
        ar.root[t] = 0;
        ar.used[t] = used;
        atomicMax(max_live, used);
    }
    const int want = (p.alpha > 0.0f) ? nE : 0;                        // apply_root_noise, MCTS.h:113-132
    if (want == 0 && lane < nE) ncold[noff + lane].noise = 0.0f;
    if (!dev_noise) {
        if (lane == 0) noise_req[t] = want;
    } else if (want > 0 && replay_noise != nullptr) {
        // recorded draws instead of the generator (az_mcts_dev_replay): row t, edge order
        if (lane < want) ncold[noff + lane].noise = replay_noise[static_cast<size_t>(t) * G::ACTIONS + lane];
    } else if (want > 0) {
        float g = 0.0f;
        if (lane < want) {
            DevRng rng(p.seed, *p.call_ptr, static_cast<uint64_t>(t), static_cast<uint64_t>(lane) + 128);
            g = rng.gamma(p.alpha);
        }
        const float sum = wave_ordered_sum(g, want);   // lanes >= want hold 0
        if (lane < want) ncold[noff + lane].noise = g * (1.0f / (sum + 1e-8f));
    }
}

template <class G>
__global__ void __launch_bounds__(WAVE) k_apply_noise(TreeArena ar, const int32_t *noise_req, const float *noise)
{
    constexpr int L = G::LANES;
    const int sub = threadIdx.x % L;
    const int tree = blockIdx.x * (WAVE / L) + threadIdx.x / L;
    if (tree >= ar.B) return;
    const int nv = noise_req[tree];
    if (nv <= 0 || sub >= nv) return;
    const HotRec *hot = ar.hot + tree_base(ar, tree);
    ColdRec *cold = ar.cold + tree_base(ar, tree);
    const int off = hot[ar.root[tree]].child_off;
    cold[off + sub].noise = noise[static_cast<size_t>(tree) * G::ACTIONS + sub];
}

// ------------------------------------------------------------------ root queries

// get_counts (MCTS.h:617-630) and get_root_stats (MCTS.h:637-673).  Lane e scatters the values
// of edge e into the slot of its action; the slots of actions that have no edge are zeroed by
// other writes to DISJOINT addresses (presence comes from a group ballot), so no two lanes
// ever store to the same word.
template <class G, bool STATS>
__global__ void __launch_bounds__(WAVE) k_root_query(TreeArena ar, int32_t *counts, float *stats)
{
    constexpr int L = G::LANES, A = G::ACTIONS;
    const int lane = threadIdx.x;
    const int sub = lane % L;
    const int tree = blockIdx.x * (WAVE / L) + lane / L;
    const bool live = tree < ar.B;
    const int t = live ? tree : 0;
    const HotRec *hot = ar.hot + tree_base(ar, t);
    const ColdRec *cold = ar.cold + tree_base(ar, t);
    const int root = ar.root[t];
    const HotRec R = hot[root];
    const bool expanded = (R.meta & META_EXPANDED) != 0;
    const int E = expanded ? static_cast<int>((R.meta & META_NEDGE_MASK) >> META_NEDGE_SHIFT) : 0;
    HotRec c = empty_rec();
    ColdRec cc;
    cc.w_draw = 0.f; cc.noise = 0.f; cc.parent = -1; cc.reserved = 0;
    const bool has = live && sub < E;
    if (has) {
        c = hot[R.child_off + sub];
        if (STATS) cc = cold[R.child_off + sub];
    }
    const int my_action = has ? static_cast<int>(c.meta & META_ACTION_MASK) : -1;
    // which actions own an edge: squares/columns 0..63 in a mask, action 64 (pass) separately
    const unsigned long long low = group_ballot<L>(has && my_action < 64, lane);
    unsigned long long present = 0;
    for (unsigned long long m = low; m; m &= m - 1) {
        const int e = __ffsll(m) - 1;
        present |= 1ull << __shfl(my_action, e, L);
    }
    const bool pass_present = group_ballot<L>(has && my_action == 64, lane) != 0;
    if (!live) return;
    const bool exists = has && (c.meta & META_EXISTS);

    if (!STATS) {
        int32_t *o = counts + static_cast<size_t>(t) * A;
        if (has) o[my_action] = exists ? c.n_visits : 0;
        for (int a = sub; a < A; a += L) {
            const bool pres = a < 64 ? ((present >> a) & 1ull) : pass_present;
            if (!pres) o[a] = 0;
        }
        return;
    }
    float *o = stats + static_cast<size_t>(t) * G::STATS;
    const float u3 = 1.f / 3;
    if (sub == 0) {
        const ColdRec rc = cold[root];
        const bool hv = R.n_visits != 0;
        const float inv = hv ? 1.0f / static_cast<float>(R.n_visits) : 0.0f;
        const float d = hv ? rc.w_draw * inv : u3;
        const float p1 = hv ? R.w_p1 * inv : u3;
        const float p2 = hv ? R.w_p2 * inv : u3;
        o[0] = static_cast<float>(R.n_visits);
        o[1] = (R.meta & META_TURN_P1) ? (p1 - p2) : (p2 - p1);
        o[2] = mean_m(R.n_visits, R.m_sum);
        o[3] = d; o[4] = p1; o[5] = p2;
    }
    if (has) {
        float *slot = o + 6 + my_action * 8;
        const bool hv = exists && c.n_visits != 0;
        const float inv = hv ? 1.0f / static_cast<float>(c.n_visits) : 0.0f;
        const float d = exists ? (hv ? cc.w_draw * inv : u3) : 0.0f;
        const float p1 = exists ? (hv ? c.w_p1 * inv : u3) : 0.0f;
        const float p2 = exists ? (hv ? c.w_p2 * inv : u3) : 0.0f;
        float mm = exists ? mean_m(c.n_visits, c.m_sum) : 0.0f;
        if (G::AUX_NEGATE && exists) mm = -mm;                        // MCTS.h:662-664
        slot[0] = exists ? static_cast<float>(c.n_visits) : 0.0f;
        slot[1] = exists ? ((c.meta & META_TURN_P1) ? (p1 - p2) : (p2 - p1)) : 0.0f;
        slot[2] = c.prior;
        slot[3] = cc.noise;
        slot[4] = mm;
        slot[5] = d; slot[6] = p1; slot[7] = p2;
    }
    for (int a = sub; a < A; a += L) {
        const bool pres = a < 64 ? ((present >> a) & 1ull) : pass_present;
        if (!pres) {
            float *slot = o + 6 + a * 8;
#pragma unroll
            for (int q = 0; q < 8; ++q) slot[q] = 0.0f;
        }
    }
}

// ------------------------------------------------------------------ random-playout evaluator

// RolloutEvaluator::evaluate_single (RolloutEvaluator.h:23-48) for the leaves of one plain
// selection: uniform policy (all ones), value = result of a uniformly random playout from
// the leaf, auxiliary value 0.  One thread per tree; moves come from the device generator.
template <class G>
__global__ void __launch_bounds__(256) k_rollout(LeafBuf lf, SearchParams p, int B, float *policy, float *d,
                                                 float *p1w, float *p2w, float *ml, uint8_t *is_term)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B) return;
    const uint8_t fl = lf.flags[t];
    const bool term = (fl & LEAF_TERMINAL) != 0;
    int code = (fl >> LEAF_RESULT_SHIFT) & 3;
    if (!term) {
        GameState s;
        s.bb0 = lf.bb0[t]; s.bb1 = lf.bb1[t]; s.turn = lf.turn[t]; s.aux = lf.aux[t];
        code = random_playout<G>(s, p.seed, *p.call_ptr, static_cast<uint64_t>(t));
    }
    is_term[t] = term ? 1 : 0;
    d[t] = code == 0 ? 1.0f : 0.0f;
    p1w[t] = code == 1 ? 1.0f : 0.0f;
    p2w[t] = code == 2 ? 1.0f : 0.0f;
    ml[t] = 0.0f;
    for (int a = 0; a < G::ACTIONS; ++a) policy[static_cast<size_t>(t) * G::ACTIONS + a] = term ? 0.0f : 1.0f;
}

// ------------------------------------------------------------------ batched game step

// step + result (Connect4.h:159-203 / Othello.h:206-258) on HBM-resident positions.  `aux` is the
// game's small integer carried from ply to ply (Othello: consecutive passes - the GAME remembers
// them although a tree forgets them at every import); nullptr: derived as an import derives it.
template <class G>
__global__ void __launch_bounds__(256) k_game_step(uint64_t *bb0, uint64_t *bb1, int32_t *turns, int32_t *aux,
                                                   const int32_t *actions, uint8_t *done, int32_t *winner,
                                                   int64_t n, int reset_finished)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int a = actions[i];
    if (a < 0 || a >= G::ACTIONS) { done[i] = 0; winner[i] = 0; return; }
    GameState s;
    s.bb0 = bb0[i]; s.bb1 = bb1[i]; s.turn = turns[i];
    s.aux = aux != nullptr ? aux[i] : G::root_aux(s.bb0, s.bb1);
    G::step(s, a);
    const int res = G::result(s);
    const bool fin = res >= 0;
    done[i] = fin ? 1 : 0;
    winner[i] = res == 1 ? 1 : (res == 2 ? -1 : 0);
    if (fin && reset_finished) G::start(s);
    bb0[i] = s.bb0; bb1[i] = s.bb1; turns[i] = s.turn;
    if (aux != nullptr) aux[i] = s.aux;
}

// ------------------------------------------------------------------ the device driver's ply tail

// Root visit counts -> move, for a driver whose temperature is exactly 1 (player.py:348-371 with the schedule of
// game.py:55-63): what the driver's torch chain computes, value for value.  The weights are the positive counts
// as floats (a row without one: all ones), the sampled move is the arg-max of weight / q over the row with q the
// caller's exponential draws - the form torch.multinomial gives one draw per row - and the greedy move the arg-max
// of the counts; the lowest index wins a tie in both.  hot_early / hot_late: whether the temperature in force
// before / from ply `decay_moves` (<= 0: always the early one) is above the greedy threshold.  dead: slots that
// get -1 (nullptr: none).  One thread per game.
template <class G>
__global__ void __launch_bounds__(256) k_ply_pick(const int32_t *__restrict__ counts, const float *__restrict__ q,
                                                  const int32_t *__restrict__ ply, const uint8_t *__restrict__ dead,
                                                  int32_t *__restrict__ actions, int n, int decay_moves, int hot_early,
                                                  int hot_late)
{
    constexpr int A = G::ACTIONS;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (dead != nullptr && dead[i]) { actions[i] = -1; return; }
    const int32_t *c = counts + static_cast<size_t>(i) * A;
    const float *e = q + static_cast<size_t>(i) * A;
    bool any = false;
    int greedy = 0, gbest = c[0];
    for (int a = 0; a < A; ++a) {
        const int v = c[a];
        any = any || v > 0;
        if (v > gbest) { gbest = v; greedy = a; }
    }
    int sampled = 0;
    float sbest = 0.0f;
    for (int a = 0; a < A; ++a) {
        const int v = c[a];
        const float w = any ? (v > 0 ? static_cast<float>(v) : 0.0f) : 1.0f;
        const float r = __fdiv_rn(w, e[a]);
        if (a == 0 || r > sbest) { sbest = r; sampled = a; }
    }
    const bool hot = (decay_moves <= 0 || ply[i] < decay_moves) ? hot_early != 0 : hot_late != 0;
    actions[i] = hot ? sampled : greedy;
}

// What follows the re-rooting, in one launch: k_game_step's step and result, the restart of a finished game
// (refill) or its slot going dead (no refill), the reset of its tree (k_reset_masked), the ply counters and the
// running totals {positions, games, P1 wins, P2 wins, draws} (+n positions per call, as the driver counts them).
// A slot whose action is out of range (a dead slot's -1) is left as it is with done = 0.  One thread per game;
// the four counts are summed per workgroup and reach `totals` with one atomic each.
template <class G>
__global__ void __launch_bounds__(256) k_ply_advance(TreeArena ar, uint64_t *bb0, uint64_t *bb1, int32_t *turns,
                                                     int32_t *aux, const int32_t *actions, uint8_t *done,
                                                     int32_t *winner, int32_t *ply, uint8_t *dead,
                                                     unsigned long long *totals, int n, int refill)
{
    __shared__ int s_cnt[4][4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool fin = false;
    int w = 0;
    if (i < n) {
        const int a = actions[i];
        if (a >= 0 && a < G::ACTIONS) {
            GameState s;
            s.bb0 = bb0[i]; s.bb1 = bb1[i]; s.turn = turns[i]; s.aux = aux[i];
            G::step(s, a);
            const int res = G::result(s);
            fin = res >= 0;
            w = res == 1 ? 1 : (res == 2 ? -1 : 0);
            if (fin && refill) G::start(s);
            bb0[i] = s.bb0; bb1[i] = s.bb1; turns[i] = s.turn; aux[i] = s.aux;
        }
        done[i] = fin ? 1 : 0;
        winner[i] = w;
        const bool was_dead = dead[i] != 0;
        int pl = ply[i] + (was_dead ? 0 : 1);
        if (fin) {
            write_fresh_root(ar.hot + tree_base(ar, i), ar.cold + tree_base(ar, i));
            ar.root[i] = 0;
            ar.used[i] = 1;
            if (refill) pl = 0; else dead[i] = 1;
        }
        ply[i] = pl;
    }
    const int c0 = __popcll(__ballot(fin)), c1 = __popcll(__ballot(fin && w == 1));
    const int c2 = __popcll(__ballot(fin && w == -1)), c3 = __popcll(__ballot(fin && w == 0));
    if (lane == 0) { s_cnt[wave][0] = c0; s_cnt[wave][1] = c1; s_cnt[wave][2] = c2; s_cnt[wave][3] = c3; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        const int sum = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
        if (sum) atomicAdd(totals + 1 + k, static_cast<unsigned long long>(sum));
    }
    if (blockIdx.x == 0 && threadIdx.x == 4) atomicAdd(totals, static_cast<unsigned long long>(n));
}

// legal actions of HBM-resident positions, one byte per action (env_common.h `valid_mask()`)
template <class G>
__global__ void __launch_bounds__(256) k_game_valid_mask(const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns,
                                                         const int32_t *aux, uint8_t *mask, int64_t n)
{
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t i = gid / G::ACTIONS;
    const int a = static_cast<int>(gid - i * G::ACTIONS);
    if (i >= n) return;
    GameState s;
    s.bb0 = bb0[i]; s.bb1 = bb1[i]; s.turn = turns[i];
    s.aux = aux != nullptr ? aux[i] : G::root_aux(s.bb0, s.bb1);
    mask[gid] = G::valid_in_frame(s, 0, a) ? 1 : 0;
}

__global__ void k_bump_call(uint64_t *ctr, uint64_t amount) { *ctr += amount; }

}  // namespace

// ------------------------------------------------------------------ launchers

void launch_import(int game, const int8_t *boards, const int32_t *turns, RootState rs, int B, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_import<G>, dim3((B + 255) / 256), dim3(256), 0, s, boards, turns, rs, B));
}

void launch_set_roots(int game, const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns, RootState rs,
                      int B, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_set_roots<G>, dim3((B + 255) / 256), dim3(256), 0, s, bb0, bb1, turns, rs, B));
}

void launch_bump_call(uint64_t *call_ctr, hipStream_t s, uint64_t amount)
{
    hipLaunchKernelGGL(k_bump_call, dim3(1), dim3(1), 0, s, call_ctr, amount);
}

void launch_export(int game, LeafBuf lf, SearchParams p, int n_leaves, bool gen_sym, int8_t *boards,
                   uint8_t *valid_mask, float *features, hipStream_t s)
{
    AZ_DISPATCH(game, {
        const int64_t threads = static_cast<int64_t>(n_leaves) * G::CELLS;
        hipLaunchKernelGGL(k_export<G>, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, lf, p,
                           n_leaves, gen_sym ? 1 : 0, boards, valid_mask, features);
    });
}

void launch_leaf_prep(int game, LeafBuf lf, SearchParams p, int n_leaves, bool gen_sym, uint8_t *valid_mask, int32_t *idx,
                      int64_t *count, int *err, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_leaf_prep<G>, dim3((n_leaves + 1023) / 1024), dim3(1024), 0, s, lf, p, n_leaves,
                                         gen_sym ? 1 : 0, valid_mask, idx, reinterpret_cast<long long *>(count), err));
}

void launch_prune(int game, TreeArena ar, SearchParams p, const int32_t *actions, int32_t *noise_req,
                  bool dev_noise, hipStream_t s, const float *replay_noise, int *max_live, int *err, int compact_above)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_prune<G>, dim3(static_cast<unsigned>(ar.B)), dim3(WAVE), 0, s, ar, p,
                                         actions, noise_req, dev_noise ? 1 : 0, replay_noise, max_live, err, compact_above));
}

void launch_apply_noise(int game, TreeArena ar, const int32_t *noise_req, const float *noise, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_apply_noise<G>, dim3(grid_for(ar.B, WAVE / G::LANES)), dim3(WAVE), 0, s, ar,
                                         noise_req, noise));
}

void launch_reset_masked(TreeArena ar, const uint8_t *mask, hipStream_t s)
{
    hipLaunchKernelGGL(k_reset_masked, dim3((ar.B + 255) / 256), dim3(256), 0, s, ar, mask);
}

void launch_counts(int game, TreeArena ar, int32_t *counts, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL((k_root_query<G, false>), dim3(grid_for(ar.B, WAVE / G::LANES)), dim3(WAVE), 0,
                                         s, ar, counts, static_cast<float *>(nullptr)));
}

void launch_root_stats(int game, TreeArena ar, float *stats, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL((k_root_query<G, true>), dim3(grid_for(ar.B, WAVE / G::LANES)), dim3(WAVE), 0,
                                         s, ar, static_cast<int32_t *>(nullptr), stats));
}

void launch_init_trees(TreeArena ar, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_trees, dim3((ar.B + 255) / 256), dim3(256), 0, s, ar);
}

void launch_rollout(int game, LeafBuf lf, SearchParams p, int B, float *policy, float *d, float *p1w, float *p2w,
                    float *ml, uint8_t *is_term, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_rollout<G>, dim3((B + 255) / 256), dim3(256), 0, s, lf, p, B, policy, d, p1w,
                                         p2w, ml, is_term));
}

void launch_game_step(int game, uint64_t *bb0, uint64_t *bb1, int32_t *turns, int32_t *aux, const int32_t *actions,
                      uint8_t *done, int32_t *winner, int64_t n, bool reset_finished, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_game_step<G>, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s,
                                         bb0, bb1, turns, aux, actions, done, winner, n, reset_finished ? 1 : 0));
}

void launch_ply_pick(int game, const int32_t *counts, const float *q, const int32_t *ply, const uint8_t *dead,
                     int32_t *actions, int n, int decay_moves, bool hot_early, bool hot_late, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_ply_pick<G>, dim3((n + 255) / 256), dim3(256), 0, s, counts, q, ply, dead,
                                         actions, n, decay_moves, hot_early ? 1 : 0, hot_late ? 1 : 0));
}

void launch_ply_advance(int game, TreeArena ar, uint64_t *bb0, uint64_t *bb1, int32_t *turns, int32_t *aux,
                        const int32_t *actions, uint8_t *done, int32_t *winner, int32_t *ply, uint8_t *dead,
                        int64_t *totals, bool refill, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_ply_advance<G>, dim3((ar.B + 255) / 256), dim3(256), 0, s, ar, bb0, bb1,
                                         turns, aux, actions, done, winner, ply, dead,
                                         reinterpret_cast<unsigned long long *>(totals), ar.B, refill ? 1 : 0));
}

void launch_game_valid_mask(int game, const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns, const int32_t *aux,
                            uint8_t *mask, int64_t n, hipStream_t s)
{
    AZ_DISPATCH(game, hipLaunchKernelGGL(k_game_valid_mask<G>, dim3(static_cast<unsigned>((n * G::ACTIONS + 255) / 256)),
                                         dim3(256), 0, s, bb0, bb1, turns, aux, mask, n));
}

}  // namespace az
