// engine_internal.h - what the host-side translation units of libaz_mcts.so share: the error type, the device
// buffers, the engine object and the small helpers of the C ABI's entry points.  Nothing here is exported as a
// C symbol; the shared pieces live in az::host, as the launchers of kernels.h live in az.  Included by engine.hip,
// engine_host.hip, engine_dev.hip, selfplay_driver.hip and match_driver.hip, and for the error type and the entry points'
// helpers by train_kernels.hip and optim_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "az_mcts.h"
#include "az_nn.h"
#include "host_rng.h"
#include "kernels.h"
#include "games.h"

namespace az::host {

// the text behind az_last_error(): one object per thread, whichever translation unit failed (defined in engine.hip)
extern thread_local std::string g_last_error;

struct AzError : std::runtime_error {
    int code;
    AzError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

inline void hip_check(hipError_t e, const char *what)
{
    if (e != hipSuccess)
        throw AzError(AZ_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_OK(x) hip_check((x), #x)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void ensure(size_t count, bool zero = false)
    {
        if (count <= n) return;
        if (p) HIP_OK(hipFree(p));
        p = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T)));
        n = count;
        if (zero) HIP_OK(hipMemset(p, 0, count * sizeof(T)));
    }
};

struct LeafStore {
    DevBuf<int32_t> slot, turn, aux, path_len, path, sym;
    DevBuf<uint64_t> bb0, bb1;
    DevBuf<uint8_t> flags, nvalid;
    int max_path = az::C4_MAX_PATH;
    void ensure(size_t leaves)
    {
        const bool grow = leaves > slot.n;
        slot.ensure(leaves); turn.ensure(leaves); aux.ensure(leaves, true); bb0.ensure(leaves); bb1.ensure(leaves);
        sym.ensure(leaves, true); nvalid.ensure(leaves, true);
        if (grow) {
            flags.ensure(leaves, true);
            path_len.ensure(leaves, true);   // 0 == "no descent recorded" (current_leaf_idx == -1)
            path.ensure(leaves * max_path);
        }
    }
    az::LeafBuf view()
    {
        az::LeafBuf v;
        v.slot = slot.p; v.bb0 = bb0.p; v.bb1 = bb1.p; v.turn = turn.p; v.aux = aux.p; v.nvalid = nvalid.p;
        v.flags = flags.p; v.path_len = path_len.p; v.path = path.p; v.sym = sym.p;
        return v;
    }
};

// event pairs around one kind of kernel
struct EventRing {
    std::vector<hipEvent_t> start, stop;
    size_t used = 0;
    ~EventRing()
    {
        for (auto e : start) (void)hipEventDestroy(e);
        for (auto e : stop) (void)hipEventDestroy(e);
    }
    void allocate(size_t n)
    {
        while (start.size() < n) {
            hipEvent_t a, b;
            HIP_OK(hipEventCreate(&a));
            HIP_OK(hipEventCreate(&b));
            start.push_back(a); stop.push_back(b);
        }
    }
    bool begin(hipStream_t s)
    {
        if (used >= start.size()) return false;
        // an event recorded into a graph under capture has no timestamp to read back
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone) return false;
        HIP_OK(hipEventRecord(start[used], s));
        return true;
    }
    void end(hipStream_t s) { HIP_OK(hipEventRecord(stop[used], s)); ++used; }
    void read(double &ms, int64_t &n)
    {
        ms = 0.0; n = 0;
        for (size_t i = 0; i < used; ++i) {
            float t = 0.f;
            HIP_OK(hipEventElapsedTime(&t, start[i], stop[i]));
            ms += t; ++n;
        }
        used = 0;
    }
};

// static geometry of a game as the host needs it
struct Geo {
    int actions, cells, rows, cols, stats, max_path, sym_choices;
    int max_edges;      // most legal moves a position can have = records an expansion can append (Othello: 33)
    int max_plies;      // the longest game in plies: 42 stones; Othello: 60 stones + passes, never two in a row before the end
};

inline Geo geo_of(int game)
{
    if (game == AZ_GAME_OTHELLO)
        return Geo{az::OT_ACTIONS, az::OT_CELLS, 8, 8, az::OT_STATS, az::OT_MAX_PATH, 4, 33, 126};
    return Geo{az::C4_ACTIONS, az::C4_CELLS, az::C4_ROWS, az::C4_COLS, az::C4_STATS, az::C4_MAX_PATH, 2, 7, 42};
}

inline bool known_game(int game) { return game == AZ_GAME_CONNECT4 || game == AZ_GAME_OTHELLO; }

inline az::GameState start_state(int game)
{
    az::GameState st;
    if (game == AZ_GAME_CONNECT4) az::Connect4Dev::start(st); else az::OthelloDev::start(st);
    return st;
}

template <class F>
int guarded(F &&f)
{
    try {
        f();
        return AZ_OK;
    } catch (const AzError &e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return AZ_ERR_DEVICE;
    }
}

inline void require(bool ok, const std::string &msg)
{
    if (!ok) throw AzError(AZ_ERR_ARG, msg);
}

// a device address an entry point may hand a kernel: not null, and a multiple of `to` bytes
inline bool aligned(const void *p, uintptr_t to) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % to == 0; }

// the status of a C ABI call made from inside another one: its failure, text included, becomes the caller's
inline void check_rc(int rc)
{
    if (rc != AZ_OK) throw AzError(rc, g_last_error);
}

// What a driver of whole plies (self-play, matches) keeps between its calls besides the games themselves:
// an optional tape of recorded moves, one row of B actions per ply, and two events for a bounded run-ahead.
struct PlyDriver {
    const int32_t *tape = nullptr;
    int64_t tape_plies = 0, tape_next = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};

    ~PlyDriver()
    {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void create_events() { for (auto &e : ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    void set(const int32_t *actions, int64_t n_plies) { tape = actions; tape_plies = actions ? n_plies : 0; tape_next = 0; }
    // who: the driver's prefix in the C ABI ("az_selfplay", "az_match")
    void require(const char *who) const
    {
        if (tape != nullptr && tape_next >= tape_plies)
            throw AzError(AZ_ERR_STATE, std::string(who) + ": the action tape (" + who + "_set_action_tape) is exhausted");
    }
    const int32_t *row(int B) const { return tape != nullptr ? tape + tape_next * B : nullptr; }
    void advance() { if (tape != nullptr) ++tape_next; }
    // bounded run-ahead: the host may be one ply ahead of the device (ply: the number of plies finished)
    void mark(int64_t ply, hipStream_t s)
    {
        const int slot = static_cast<int>(ply & 1);
        HIP_OK(hipEventRecord(ev[slot], s));
        ev_used[slot] = true;
        if (ev_used[slot ^ 1]) HIP_OK(hipEventSynchronize(ev[slot ^ 1]));
    }
};

}  // namespace az::host
// this header serves the host translation units only, and all of them are written in these names
using namespace az::host;

struct az_mcts {
    int game = AZ_GAME_CONNECT4;
    Geo geo = geo_of(AZ_GAME_CONNECT4);
    int B = 0;
    int device = 0;
    az_search_config cfg;

    // trees
    DevBuf<az::HotRec> hot;
    DevBuf<az::ColdRec> cold;
    DevBuf<int32_t> root, used;
    DevBuf<uint8_t> half;     // which of its two arena halves a tree lives in (tree_layout.h)
    int64_t S = 0;            // records per half
    int64_t used_bound = 1;   // host-side upper bound of max(used[])
    // What the trees occupy after a re-rooting, reported by the prune kernel without stalling the host:
    // prune number q leaves its maximum in live_ring[q % 8] (pinned host memory) through an async copy;
    // growth_after[q % 8] sums the room handed out by ensure_room since that prune was issued, so that
    // `arrived value + growth since` is an upper bound of max(used[]) again.
    DevBuf<int> max_live;
    volatile int *live_ring = nullptr;
    int64_t prune_seq = 0;
    int64_t ring_seq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t growth_after[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t last_extra = 0;   // room asked for by the last ensure_room call
    int64_t growth_since_prune = 0;   // room handed out since the previous re-rooting = one ply's worst-case growth,
                                      // whether it was asked for in one call (device loop) or in one call per
                                      // backprop (host entry points)
    int64_t epoch = 0;        // bumped whenever a buffer the dev_* kernels address moves

    // roots of the current call
    DevBuf<uint64_t> r_bb0, r_bb1;
    DevBuf<int32_t> r_turn, r_last;

    LeafStore vl_leaf, plain_leaf;
    int vl_stride = 0;        // K of the last VL selection (flat = tree*K + k)
    bool last_select_vl = false;

    // c_puct table
    DevBuf<float> tab;
    float tab_c_init = NAN, tab_c_base = NAN;
    DevBuf<float> term_tab;   // Othello terminal_aux by diff*turn + 64
    float term_tab_scale = NAN;

    DevBuf<unsigned long long> counters;
    DevBuf<int> err;
    int *err_host = nullptr;  // pinned copy of `err` (az_mcts_dev_check)
    DevBuf<uint64_t> call_ctr;
    // recorded draws that stand in for the device generator (az_mcts_dev_replay; parity tests)
    const int32_t *replay_sym = nullptr;
    int64_t replay_stride = 0, replay_calls = 0, replay_next = 0;
    const float *replay_noise = nullptr;
    // device transposition table of evaluator outputs (tt_kernels.hip)
    DevBuf<uint8_t> tt_entries;     // 2^n entries of az::tt_entry_bytes(game) bytes
    DevBuf<unsigned long long> tt_stats;
    DevBuf<uint64_t> tt_keys;
    uint64_t tt_mask = 0;
    int64_t select_launches = 0, backprop_launches = 0;
    const float *noise_eps_tree = nullptr;     // caller-owned device array (az_mcts_dev_set_noise_epsilons)
    // leaf batch of az_mcts_dev_search: evaluator inputs, outputs, compact row list, activations
    DevBuf<float> ev_feat, ev_probs, ev_wdl, ev_ml;
    DevBuf<uint8_t> ev_mask, ev_scratch;
    DevBuf<int32_t> ev_rows;
    DevBuf<int64_t> ev_nrows;
    // one chunk of az_mcts_dev_tt_refresh
    DevBuf<float> rf_probs, rf_wdl, rf_ml;
    DevBuf<uint8_t> rf_mask, rf_scratch;
    DevBuf<uint64_t> rf_bb0, rf_bb1;
    DevBuf<int32_t> rf_rows, rf_turn, rf_sym;
    DevBuf<int64_t> rf_count;
    DevBuf<uint64_t> rf_keys;
    bool profiling = false;
    int profile_stride = 1;      // time every profile_stride-th launch of a kind
    int64_t profile_seen[2] = {0, 0};
    EventRing ev_select, ev_backprop;
    const char *timed_select_kernel = "";   // the kernel behind the newest timed selection launch (az_mcts_timed_select_kernel)

    // IO buffers of the host entry points
    DevBuf<int8_t> io_boards_in, io_boards_out;
    DevBuf<int32_t> io_turns_in, io_sym_in, io_actions, io_noise_req, io_counts;
    DevBuf<uint8_t> io_mask_out, io_is_term, io_reset_mask;
    DevBuf<float> io_policy, io_d, io_p1, io_p2, io_ml, io_noise, io_stats;

    // host generator and what it needs to know between search and backprop
    az::HostRng rng;
    uint64_t dev_seed = 0x5eed;
    std::vector<uint8_t> stash_flags_vl, stash_flags_plain;
    std::vector<uint8_t> stash_root_nv;   // open columns of each root (valid moves of an unexpanded root)
    std::vector<uint8_t> pending_reset;
    bool any_pending_reset = false;

    static constexpr int kCpuctTab = 1 << 16;

    az::TreeArena arena()
    {
        az::TreeArena a;
        a.hot = hot.p; a.cold = cold.p; a.half = half.p; a.root = root.p; a.used = used.p; a.S = S; a.B = B;
        return a;
    }
    az::RootState roots()
    {
        az::RootState r;
        r.bb0 = r_bb0.p; r.bb1 = r_bb1.p; r.turn = r_turn.p; r.aux = r_last.p;
        return r;
    }

    void ensure_table()
    {
        // Othello.h:260-266 with the host libm: atanf(raw / scale) * (2.0f / 3.14159265f)
        if (!term_tab.p || cfg.score_scale != term_tab_scale) {
            std::vector<float> h(129);
            for (int i = 0; i < 129; ++i) {
                const float raw = static_cast<float>(i - 64);
                h[i] = std::atan(raw / cfg.score_scale) * (2.0f / 3.14159265f);
            }
            if (!term_tab.p) ++epoch;
            term_tab.ensure(129);
            HIP_OK(hipMemcpy(term_tab.p, h.data(), sizeof(float) * 129, hipMemcpyHostToDevice));
            term_tab_scale = cfg.score_scale;
        }
        // logf through the host libm, float arithmetic in the reference's order (MCTS.h:213-214)
        if (tab.p && cfg.c_init == tab_c_init && cfg.c_base == tab_c_base) return;
        // second half: sqrtf(parent_n) - correctly rounded on either side, tabulated to take ~17 instructions
        // out of a level of the Connect4 selection kernels
        std::vector<float> h(2 * kCpuctTab);
        const float c_init = cfg.c_init, c_base = cfg.c_base;
        for (int n = 0; n < kCpuctTab; ++n) {
            const float parent_n = static_cast<float>(n);
            h[n] = c_init + std::log((parent_n + c_base + 1.0f) / c_base);
            h[kCpuctTab + n] = std::sqrt(parent_n);
        }
        if (!tab.p) ++epoch;
        tab.ensure(2 * kCpuctTab);
        HIP_OK(hipMemcpy(tab.p, h.data(), sizeof(float) * 2 * kCpuctTab, hipMemcpyHostToDevice));
        tab_c_init = c_init; tab_c_base = c_base;
    }

    az::SearchParams params()
    {
        ensure_table();
        az::SearchParams p;
        p.c_init = cfg.c_init; p.c_base = cfg.c_base; p.noise_eps = cfg.noise_epsilon;
        p.fpu_reduction = cfg.fpu_reduction; p.mlh_slope = cfg.mlh_slope; p.mlh_cap = cfg.mlh_cap;
        p.value_decay = cfg.value_decay; p.alpha = cfg.dirichlet_alpha;
        p.score_utility_factor = cfg.score_utility_factor; p.term_aux_tab = term_tab.p;
        p.vl_count = cfg.vl_count; p.use_symmetry = cfg.use_symmetry ? 1 : 0;
        p.cpuct_tab = tab.p; p.tab_n = kCpuctTab;
        p.seed = dev_seed; p.call_ptr = call_ctr.p;
        p.noise_eps_tree = noise_eps_tree;
        return p;
    }

    void reset_all_trees()
    {
        std::fill(pending_reset.begin(), pending_reset.end(), 1);
        any_pending_reset = true;
    }

    void flush_resets(hipStream_t s)
    {
        if (!any_pending_reset) return;
        HIP_OK(hipStreamSynchronize(s));          // an earlier reset launch may still be reading the mask
        io_reset_mask.ensure(B);
        HIP_OK(hipMemcpy(io_reset_mask.p, pending_reset.data(), B, hipMemcpyHostToDevice));
        az::launch_reset_masked(arena(), io_reset_mask.p, s);
        std::fill(pending_reset.begin(), pending_reset.end(), 0);
        any_pending_reset = false;
    }

    int64_t true_max_used()
    {
        std::vector<int32_t> h(B);
        HIP_OK(hipMemcpy(h.data(), used.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
        return *std::max_element(h.begin(), h.end());
    }

    void grow(int64_t new_S)
    {
        HIP_OK(hipDeviceSynchronize());
        const int64_t keep = std::min<int64_t>(S, true_max_used());
        DevBuf<az::HotRec> nh;
        DevBuf<az::ColdRec> nc;
        nh.ensure(static_cast<size_t>(B) * 2 * new_S);
        nc.ensure(static_cast<size_t>(B) * 2 * new_S);
        // one row per half (slots are relative to a half: nothing to renumber)
        HIP_OK(hipMemcpy2D(nh.p, new_S * sizeof(az::HotRec), hot.p, S * sizeof(az::HotRec),
                           keep * sizeof(az::HotRec), static_cast<size_t>(B) * 2, hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy2D(nc.p, new_S * sizeof(az::ColdRec), cold.p, S * sizeof(az::ColdRec),
                           keep * sizeof(az::ColdRec), static_cast<size_t>(B) * 2, hipMemcpyDeviceToDevice));
        std::swap(hot.p, nh.p); std::swap(hot.n, nh.n);
        std::swap(cold.p, nc.p); std::swap(cold.n, nc.n);
        S = new_S;
        ++epoch;
    }

    // the newest re-rooting whose occupancy figure has arrived tightens the host-side bound
    void tighten_bound()
    {
        for (int64_t q = prune_seq; q > 0 && q > prune_seq - 8; --q) {
            const int v = live_ring[q % 8];
            if (ring_seq[q % 8] == q && v >= 0) {
                used_bound = std::min<int64_t>(used_bound, static_cast<int64_t>(v) + growth_after[q % 8]);
                return;
            }
        }
    }
    bool room_needs_device(int64_t extra)
    {
        if (used_bound + extra > S) tighten_bound();
        return used_bound + extra > S;
    }

    // room for `extra` more records in every tree (an expansion appends at most A records)
    void ensure_room(int64_t extra)
    {
        if (used_bound + extra > S) tighten_bound();
        if (used_bound + extra > S) {
            used_bound = true_max_used();
            if (used_bound + extra > S) grow(std::max<int64_t>(2 * S, used_bound + extra));
        }
        used_bound += extra;
        for (auto &g : growth_after) g += extra;
        last_extra = extra;
        growth_since_prune += extra;
    }

    void check_device_error()
    {
        int e = 0;
        HIP_OK(hipMemcpy(&e, err.p, sizeof(int), hipMemcpyDeviceToHost));
        if (e) {
            HIP_OK(hipMemset(err.p, 0, sizeof(int)));
            if (err_host) *err_host = 0;
            throw AzError(AZ_ERR_CAPACITY, device_error_text(e));
        }
    }
    static std::string device_error_text(int e)
    {
        std::string msg;
        if (e & az::ERR_ARENA_OVERFLOW) msg += "tree arena overflow on device (expansions were dropped)";
        if (e & az::ERR_LIST_OVERFLOW) msg += std::string(msg.empty() ? "" : "; ") + "compact leaf list overflow on device (entries were dropped)";
        if (msg.empty()) msg = "device error word " + std::to_string(e);
        return msg;
    }

    // re-rooting on `s` (k_prune: the kept subtrees move to the other arena halves); its occupancy figure
    // travels to live_ring behind it
    void prune_on(const int32_t *actions_dev, int32_t *noise_req, bool dev_noise, const float *noise_replay, hipStream_t s)
    {
        const int64_t q = ++prune_seq;
        // the slot's previous figure (prune q - 8) must have landed before the slot is handed out again
        if (ring_seq[q % 8] != 0 && live_ring[q % 8] < 0) HIP_OK(hipStreamSynchronize(s));
        live_ring[q % 8] = -1;
        ring_seq[q % 8] = q;
        growth_after[q % 8] = 0;
        HIP_OK(hipMemsetAsync(max_live.p, 0, sizeof(int), s));
        // compact the trees that could not take two more plies' worth of growth where they are
        // (AZ_COMPACT_ALWAYS=1: every tree at every re-rooting; read per call, so a test can turn it on for one engine)
        const char *const env_always = getenv("AZ_COMPACT_ALWAYS");
        const bool always = env_always != nullptr && env_always[0] == '1';
        // (one ply = what was reserved since the previous re-rooting; the host entry points reserve per backprop
        // call, so the last call's figure alone would let a tree run into the end of its half mid-search)
        const int64_t ply = std::max<int64_t>(std::max(growth_since_prune, last_extra), geo.max_edges);
        growth_since_prune = 0;
        const int64_t above = always ? 0 : std::max<int64_t>(S / 8, S - 2 * ply);
        az::launch_prune(game, arena(), params(), actions_dev, noise_req, dev_noise, s, noise_replay, max_live.p, err.p,
                         static_cast<int>(above));
        HIP_OK(hipMemcpyAsync(const_cast<int *>(&live_ring[q % 8]), max_live.p, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    ~az_mcts()
    {
        if (err_host) (void)hipHostFree(err_host);
        if (live_ring) (void)hipHostFree(const_cast<int *>(live_ring));
    }
};
